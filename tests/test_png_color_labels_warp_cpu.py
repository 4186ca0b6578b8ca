"""debig_png_decode_batch_color_labels_warp without a GPU (include/decode_png.h): the restatement
tests/png_color_label_warp_ref.py on small cases, and what the C call decides on the host alone -- every argument check (status
and unmatched left at their sentinels; the inherited checks of debig_png_decode_batch_color_labels still come first), E_WARP
with its place in the order of statuses -- and the Python keywords' refusals."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_label_ref as CR  # noqa: E402
import png_color_label_warp_ref as CW  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_warp_ref as WR  # noqa: E402
import test_png_color_labels_cpu as CC  # noqa: E402  (the descriptors and the inherited BAD_ARG cases)

BAD_ARG = -2
DUMMY = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced: the calls below never reach the device
SENTINEL = 0xABCD
U8, U16, I32, I64 = range(4)
PACK, MAP = 0, 1
CONSTANT, CLAMP = 0, 1
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class Warp(C.Structure):  # include/decode_png.h: debig_png_warp
    _fields_ = [("m", C.c_double * 6)]


class LabelWarpDesc(C.Structure):  # include/decode_png.h: debig_png_label_warp_desc
    _fields_ = [("border_mode", C.c_uint32), ("border_label", C.c_int32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_decode_batch_color_labels_warp.restype = C.c_int
    L.debig_png_decode_batch_color_labels_warp.argtypes = [C.c_void_p] * 8 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def _call(lib, files, desc, wd, out=DUMMY, boxes=None, warps="ident"):
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    st = (C.c_uint32 * n)(*[SENTINEL] * n)
    um = (C.c_uint32 * n)(*[SENTINEL] * n)
    bx = (CC.Box * n)(*[CC.Box(*b) if b else CC.Box(0, 0, 0, 0) for b in boxes]) if boxes else None
    ws = None
    if warps is not None:
        ws = (Warp * n)()
        for i, m in enumerate([IDENT] * n if warps == "ident" else warps):
            ws[i].m[:] = list(m)
    rc = lib.debig_png_decode_batch_color_labels_warp(ins, sizes, out, bx, ws, st, None, um, n, 0,
                                                      C.byref(desc) if desc is not None else None, C.byref(wd) if wd is not None else None)
    return rc, list(st), list(um)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def test_restatement_on_a_small_case():
    px = np.zeros((2, 3, 3), np.uint8)
    px[..., 0] = [[1, 2, 3], [4, 5, 6]]
    ident = WR.quantise(IDENT)
    out, miss = CW.warp_color_labels(px, (2, 3), ident, dtype="int32")
    assert out.tolist() == [[1, 2, 3], [4, 5, 6]] and miss == 0
    # one column to the right of the crop, one row below it: CONSTANT stores border_label and counts no border element ...
    colors = {1: 10, 2: 20, 4: 40}
    out, miss = CW.warp_color_labels(px, (3, 4), ident, CONSTANT, -1, None, colors, -1, "int64")
    assert out.tolist() == [[10, 20, -1, -1], [40, -1, -1, -1], [-1, -1, -1, -1]] and miss == 3  # the colours 3, 5 and 6
    # ... CLAMP repeats the edge, through the map, and counts every element that took `missing`
    out, miss = CW.warp_color_labels(px, (3, 4), ident, CLAMP, 77, None, colors, -1, "int64")
    assert out.tolist() == [[10, 20, -1, -1], [40, -1, -1, -1], [40, -1, -1, -1]] and miss == 8
    # a flip about the crop of a box, packed
    out, _ = CW.warp_color_labels(px, (2, 2), WR.quantise((-1, 0, 2, 0, 1, 0)), box=(1, 0, 2, 2), dtype="int32")
    assert out.tolist() == [[3, 2], [6, 5]]
    # composed of the two restatements it names: the identity at the crop's size is the gather
    rng = np.random.default_rng(1)
    big = rng.integers(0, 4, size=(9, 7, 3)).astype(np.uint8)
    cm = {int(k): i for i, k in enumerate(np.unique(CR.pack(big))[::2])}
    for box in (None, (2, 3, 4, 5)):
        w, h = (box[2], box[3]) if box else (7, 9)
        a, am = CW.warp_color_labels(big, (h, w), ident, CLAMP, 0, box, cm, -3, "int32")
        b, bm = CR.gather(big, (h, w), box, cm, -3, "int32")
        assert np.array_equal(a, b) and am == bm


# ---- the C call: what needs no device ----------------------------------------------------------------------------------------------

def test_argument_checks_leave_status_and_unmatched_unwritten(lib):
    f = [b"not a png", b"x"]
    untouched = (BAD_ARG, [SENTINEL] * 2, [SENTINEL] * 2)
    LW = LabelWarpDesc
    one = [CC._map([1, 2, 3])]
    pack = CC._desc()
    assert _call(lib, f, pack, LW(0, 0), warps=None) == untouched                # warps NULL
    assert _call(lib, f, pack, None) == untouched                                # warp_desc NULL
    assert _call(lib, f, pack, LW(2, 0)) == untouched                            # an unknown border mode
    u8 = CC._desc(dtype=U8, mode=MAP, missing=0, maps=one)
    u16 = CC._desc(dtype=U16, mode=MAP, missing=0, maps=one)
    for desc, wd in ((u8, LW(CONSTANT, 256)), (u8, LW(CONSTANT, -1)), (u16, LW(CONSTANT, 65536)), (u16, LW(CONSTANT, -1))):
        assert _call(lib, f, desc, wd) == untouched, (desc.dtype, wd.border_label)
    # the same values pass under CLAMP, which does not read border_label; the ranges' ends pass under CONSTANT
    reached = (0, [R.E_SIGNATURE] * 2, [0, 0])
    for desc, wd in ((u8, LW(CLAMP, 256)), (u16, LW(CLAMP, -1)), (u8, LW(CONSTANT, 255)), (u8, LW(CONSTANT, 0)),
                     (u16, LW(CONSTANT, 65535)), (pack, LW(CONSTANT, -2 ** 31)), (pack, LW(CONSTANT, 2 ** 31 - 1)),
                     (CC._desc(dtype=I32, mode=MAP, maps=one * 2), LW(CONSTANT, -1))):
        assert _call(lib, f, desc, wd) == reached, (desc.dtype, wd.border_mode, wd.border_label)
    # n == 0: nothing is checked, nothing is done
    assert lib.debig_png_decode_batch_color_labels_warp(None, None, None, None, None, None, None, None, 0, 0, None, None) == 0


def test_every_inherited_check_is_still_refused_and_comes_first(lib):
    """every BAD_ARG case of debig_png_decode_batch_color_labels, with valid warp arguments -- and with warp arguments that
    would be refused themselves: the result is the same, nothing is written"""
    f = [b"not a png", b"x"]
    cases = CC.bad_arg_cases(2)
    assert len(cases) >= 30
    for name, desc, off in cases:
        out = None if off is None else DUMMY + off
        assert _call(lib, f, desc, LabelWarpDesc(0, 0), out) == (BAD_ARG, [SENTINEL] * 2, [SENTINEL] * 2), name
        assert _call(lib, f, desc, None, out, warps=None) == (BAD_ARG, [SENTINEL] * 2, [SENTINEL] * 2), name


def test_status_order_label_box_warp_then_the_file(lib):
    """E_LABEL (a 16-bit file), then E_BOX, then E_WARP, as soon as IHDR has been read: each outranks what the file holds later (a
    damaged CRC, a missing IDAT); the walk's own statuses before the end of IHDR stand"""
    rng = np.random.default_rng(4)
    rgb16 = R.encode(R.random_image(rng, 9, 7, 2, 16), 2, 16)
    rgb = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    pal = R.encode(R.random_image(rng, 9, 7, 3, 4, 5), 3, 4, palette=[(1, 2, 3)] * 5)
    rgb_crc = bytearray(rgb)
    rgb_crc[-20] ^= 1
    rgb16_crc = bytearray(rgb16)
    rgb16_crc[-20] ^= 1
    nan = (1.0, 0.0, math.nan, 0.0, 1.0, 0.0)
    big = (1.0, 32768.5, 0.0, 0.0, 1.0, 0.0)
    far = (1.0, 0.0, 0.0, 0.0, 1.0, -2.0 ** 24 - 4)
    assert all(WR.quantise(m) is None for m in (nan, big, far))
    L, B, Wp = CR.E_LABEL, CR.E_BOX, CW.E_WARP
    #        all three broken      label > warp  box > warp  warp > CRC      warp > no IDAT  warp alone  before IHDR ends
    files = [bytes(rgb16_crc),     rgb16,        pal,        bytes(rgb_crc), rgb[:40],       pal,        rgb[:30], b"\x89PNG"]
    boxes = [(0, 0, 10, 1),        None,         (3, 3, 0, 2), None,         None,           (1, 1, 8, 6), None,   None]
    warps = [nan,                  big,          far,        far,            nan,            big,        nan,      big]
    want = [L, L, B, Wp, Wp, Wp, R.E_CHUNK, R.E_SIGNATURE]
    for desc in (CC._desc(), CC._desc(dtype=U8, mode=MAP, missing=0, maps=[CC._map([1, 2])])):
        for wd in (LabelWarpDesc(CONSTANT, 0), LabelWarpDesc(CLAMP, 0)):
            assert _call(lib, files, desc, wd, boxes=boxes, warps=warps) == (0, want, [0] * len(files))
    # the same files with good boxes and matrices: only the 16-bit ones and the damaged ones keep a status decided on the host
    assert _call(lib, files[:2] + files[6:], CC._desc(), LabelWarpDesc(0, 0)) == (0, [L, L, R.E_CHUNK, R.E_SIGNATURE], [0] * 4)


# ---- Python ------------------------------------------------------------------------------------------------------------------------

def test_python_keywords_and_descriptor():
    import inspect

    from debigulator_amd import api

    p = inspect.signature(api.png_decode_batch_color_labels).parameters
    assert [(k, p[k].default) for k in list(p)[-3:]] == [("warp", None), ("border", "constant"), ("border_label", None)]
    # the ctypes mirrors are the C structs
    assert C.sizeof(api.PngLabelWarpDesc) == C.sizeof(LabelWarpDesc) == 8 and C.sizeof(api.PngWarp) == C.sizeof(Warp) == 48
    # border / border_label belong to a warp: refused without one, before any device is looked for
    for kw in (dict(border="clamp"), dict(border_label=255), dict(border="constant", border_label=0)):
        with pytest.raises(ValueError, match="need warp"):
            api.png_decode_batch_color_labels([b""], (4, 4), **kw)
    # with a warp the rules of png_label_warp_desc and _png_warps hold, again before any device is looked for
    for kw in (dict(border="mirror"), dict(border="clamp", border_label=3), dict(border_label=256, dtype="uint8", colors={(1, 2, 3): 0}, missing=0),
               dict(border_label=-1, dtype="uint16", colors={(1, 2, 3): 0}, missing=0), dict(border_label=2 ** 31)):
        with pytest.raises(ValueError):
            api.png_decode_batch_color_labels([b""], (4, 4), warp=[None], **kw)
    with pytest.raises(ValueError, match="one entry"):
        api.png_decode_batch_color_labels([b"", b""], (4, 4), warp=[None])
    with pytest.raises(ValueError, match="2 x 3"):
        api.png_decode_batch_color_labels([b""], (4, 4), warp=[(1, 0, 0, 1)])
    with pytest.raises(ValueError):
        api.png_decode_batch_color_labels([b""], (4, 4), dtype="uint8", warp=[None])  # PACK needs int32 / int64, as without a warp
