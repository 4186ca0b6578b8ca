"""debig_png_decode_batch_labels without a GPU (include/decode_png.h): the numpy restatement tests/png_label_ref.py against the
reference decoder the rest of the suite uses, its index rule against the host's NEAREST rule
(debig_png_resize_weights_filter), and what the C call decides on the host alone: the argument checks (status left at its
sentinel) and the statuses E_LABEL / E_BOX, their order included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_ref as LR  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_gpu_png_spec as G  # noqa: E402

BAD_ARG = -2
DUMMY = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced: the calls below never reach the device
NEAREST = 2
U8, U16, I32, I64 = range(4)
SENTINEL = 0xABCD


class LabelDesc(C.Structure):  # include/decode_png.h: debig_png_label_desc
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("dtype", C.c_uint32), ("reserved", C.c_uint32),
                ("lut", C.POINTER(C.c_int32))]


class Box(C.Structure):  # include/decode_png.h: debig_png_box
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_decode_batch_labels.restype = C.c_int
    L.debig_png_decode_batch_labels.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p]
    L.debig_png_resize_weights_filter.restype = C.c_uint32
    L.debig_png_resize_weights_filter.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_uint32), C.POINTER(C.c_int16), C.c_uint32]
    return L


# ---- the restatement against the rest of the suite --------------------------------------------------------------------------

def test_labels_against_the_reference_decoder():
    """grey 8 without tRNS and grey 16: the grey channel of R.decode (its high byte for 16 bits); every palette file: the
    labels run through the file's palette are R.decode's RGBA; every other colour type: E_LABEL"""
    seen = set()
    for (ct, depth, il, trns), data in G._all_formats():
        st, lab, inf = LR.labels(data)
        est, rgba, einf = R.decode(data)
        assert est == R.OK and inf == einf
        if ct not in (0, 3):
            assert st == LR.E_LABEL and lab is None
            continue
        assert st == R.OK and lab.shape == (70, 45) and lab.dtype == np.uint32
        assert int(lab.max()) < 1 << depth
        if ct == 0 and depth == 8 and not trns:
            assert np.array_equal(lab, rgba[:, :, 0])
        elif ct == 0 and depth == 16:
            assert np.array_equal(lab >> 8, rgba[:, :, 0])
            assert (lab & 0xFF).any()  # the low byte is there
            assert LR.labels(data, "uint8")[0] == LR.E_LABEL and LR.labels(data, "int32", list(range(256)))[0] == LR.E_LABEL
            assert LR.labels(data, "uint16")[0] == R.OK
        elif ct == 3:
            pal = R._walk(data)[2][0]
            full = np.zeros((256, 4), np.uint8)
            full[: len(pal)] = pal
            assert np.array_equal(full[lab], rgba)
        seen.add((ct, depth, il))
    assert seen == {(ct, d, il) for ct in (0, 3) for d in R.DEPTHS[ct] for il in (0, 1)}


@pytest.mark.parametrize("ct", [0, 3])
def test_interlaced_equals_plain_and_the_samples(ct):
    rng = np.random.default_rng(31 + ct)
    for depth in R.DEPTHS[ct]:
        for w, h in ((1, 1), (7, 3), (45, 70)):
            n_pal = 1 << depth if ct == 3 else None
            s = R.random_image(rng, w, h, ct, depth, n_pal)
            pal = [(k, 255 - k, 7) for k in range(n_pal)] if ct == 3 else None
            a = LR.labels(R.encode(s, ct, depth, 0, palette=pal))
            b = LR.labels(R.encode(s, ct, depth, 1, palette=pal, trns=b"\x00\x01" if ct == 0 else b"\x05"))
            assert a[0] == b[0] == R.OK and b[2]["has_trns"] == 1
            assert np.array_equal(a[1], s[:, :, 0]) and np.array_equal(b[1], s[:, :, 0])


def test_palette_index_past_plte_and_walk_errors():
    bad = R.encode(np.full((5, 6, 1), 3, np.uint8), 3, 8, palette=[(1, 2, 3)] * 3)
    assert LR.labels(bad)[0] == R.E_PALETTE
    assert LR.labels(b"not a png")[0] == R.E_SIGNATURE
    for name, data, st in G._error_files():
        want = LR.E_LABEL if R._walk(data, info_only=True)[1]["color_type"] not in (0, 3) else st
        assert LR.labels(data)[0] == want, name


# ---- the index rule ---------------------------------------------------------------------------------------------------------

def _host_index(lib, cl, L, X):
    first = C.c_uint32(0xFFFFFFFF)
    w = (C.c_int16 * 4)()
    assert lib.debig_png_resize_weights_filter(NEAREST, cl, L, 0, X, C.byref(first), w, 4) == 1 and w[0] == 16384
    return first.value


def test_index_rule_is_the_nearest_filter_of_the_tensor_call(lib):
    for cl in range(1, 41):
        for L in range(1, 41):
            assert LR.index(cl, L).tolist() == [_host_index(lib, cl, L, X) for X in range(L)], (cl, L)
    cl, L = 2 ** 31 - 1, 16384  # the product needs more than 32 bits
    idx = LR.index(cl, L)
    assert idx.tolist() == [_host_index(lib, cl, L, X) for X in range(L)]
    assert (np.diff(idx) >= 0).all() and idx[0] == cl // (2 * L) and idx[-1] < cl


def test_gather_restatement_on_a_small_case():
    lab = np.arange(12, dtype=np.uint32).reshape(3, 4)
    assert np.array_equal(LR.gather(lab, (3, 4)), lab)
    assert LR.gather(lab, (1, 2)).tolist() == [[5, 7]]
    assert LR.gather(lab, (2, 2), box=(1, 1, 2, 2), lut=[-k for k in range(256)], dtype="int32").tolist() == [[-5, -6], [-9, -10]]
    assert LR.gather(lab, (3, 8), dtype="uint8")[0].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]


# ---- the C call: what needs no device -----------------------------------------------------------------------------------------

def _call(lib, files, desc, out=DUMMY, boxes=None):
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    st = (C.c_uint32 * n)(*[SENTINEL] * n)
    bx = (Box * n)(*[Box(*b) if b else Box(0, 0, 0, 0) for b in boxes]) if boxes else None
    rc = lib.debig_png_decode_batch_labels(ins, sizes, out, bx, st, None, n, 0, C.byref(desc) if desc is not None else None)
    return rc, list(st)


def _desc(out_w=8, out_h=6, dtype=I64, reserved=0, lut=None):
    d = LabelDesc(out_w=out_w, out_h=out_h, dtype=dtype, reserved=reserved)
    if lut is not None:
        d._keep = (C.c_int32 * 256)(*lut)
        d.lut = C.cast(d._keep, C.POINTER(C.c_int32))
    return d


def test_argument_checks_leave_status_unwritten(lib):
    ident = list(range(256))
    bad = [(None, DUMMY), (_desc(), None), (_desc(), DUMMY + 8), (_desc(out_w=0), DUMMY), (_desc(out_w=16385), DUMMY),
           (_desc(out_h=0), DUMMY), (_desc(out_h=16385), DUMMY), (_desc(dtype=4), DUMMY), (_desc(reserved=1), DUMMY),
           (_desc(dtype=U8, lut=ident[:255] + [256]), DUMMY), (_desc(dtype=U8, lut=[-1] + ident[1:]), DUMMY),
           (_desc(dtype=U16, lut=ident[:100] + [65536] + ident[101:]), DUMMY), (_desc(dtype=U16, lut=ident[:255] + [-1]), DUMMY)]
    for desc, out in bad:
        assert _call(lib, [b"not a png"], desc, out) == (BAD_ARG, [SENTINEL])
    # n == 0: nothing is checked, nothing is done
    assert lib.debig_png_decode_batch_labels(None, None, None, None, None, None, 0, 0, None) == 0
    # the same arguments at the edge of their ranges pass the checks and reach the file
    for desc in (_desc(out_w=16384, out_h=16384), _desc(dtype=U8, lut=ident), _desc(dtype=U16, lut=[65535] * 256),
                 _desc(dtype=I32, lut=[-1] * 256), _desc(dtype=I64, lut=[-2 ** 31] + [2 ** 31 - 1] * 255), _desc(dtype=U8)):
        assert _call(lib, [b"not a png"], desc) == (0, [R.E_SIGNATURE])
    assert _call(lib, [b"not a png"], _desc(), DUMMY + 16) == (0, [R.E_SIGNATURE])


def test_label_and_box_statuses_are_decided_on_the_host(lib):
    """E_LABEL, then E_BOX, as soon as IHDR has been read: both outrank what the file holds later (here a damaged CRC and a
    missing IDAT), and the walk's own statuses before IHDR come first"""
    rng = np.random.default_rng(4)
    rgb = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    ga = R.encode(R.random_image(rng, 9, 7, 4, 16), 4, 16)
    rgba = R.encode(R.random_image(rng, 9, 7, 6, 8), 6, 8)
    g16 = R.encode(R.random_image(rng, 9, 7, 0, 16), 0, 16)
    g8 = R.encode(R.random_image(rng, 9, 7, 0, 8), 0, 8)
    pal = R.encode(R.random_image(rng, 9, 7, 3, 4, 5), 3, 4, palette=[(1, 2, 3)] * 5)
    g8_crc = bytearray(g8)
    g8_crc[-20] ^= 1
    files = [rgb, ga, rgba, rgb, g8, pal, g8[:40], bytes(g8_crc), g8[:33]]
    boxes = [None, None, None, (0, 0, 10, 1), (0, 0, 10, 1), (3, 3, 0, 2), (8, 6, 2, 1), (0, 7, 9, 1), None]
    L, B = LR.E_LABEL, LR.E_BOX
    assert _call(lib, files, _desc(), boxes=boxes) == (0, [L, L, L, L, B, B, B, B, R.E_CHUNK])
    # a 16-bit file: E_LABEL with uint8 and with a lut (before its box is looked at), else its box decides
    for desc, want in ((_desc(dtype=U8), L), (_desc(dtype=I64, lut=list(range(256))), L), (_desc(dtype=U16), B), (_desc(), B)):
        assert _call(lib, [g16, b"\x89PNG"], desc, boxes=[(0, 0, 10, 8), None]) == (0, [want, R.E_SIGNATURE])
    for data in files[:3] + [g16]:
        assert LR.labels(data, "uint8")[0] == L


def test_python_descriptor_checks():
    from debigulator_amd import api

    d, es = api.png_label_desc((6, 8), "int32", lut=[-1] * 256)
    assert (d.out_w, d.out_h, d.dtype, d.reserved, es) == (8, 6, I32, 0, 4) and d.lut[255] == -1
    assert api.png_label_desc((1, 16384), "uint8")[1] == 1 and not api.png_label_desc((1, 1))[0].lut
    for kw in (dict(size=(0, 4)), dict(size=(4, 16385)), dict(size=(4, 4), dtype="float32"), dict(size=(4, 4), lut=[0] * 255),
               dict(size=(4, 4), dtype="uint8", lut=[256] * 256), dict(size=(4, 4), dtype="uint16", lut=[-1] * 256),
               dict(size=(4, 4), lut=[0.5] * 256)):
        with pytest.raises(ValueError):
            api.png_label_desc(**kw)
    assert api.PNG_STATUS[LR.E_LABEL] == "label"
