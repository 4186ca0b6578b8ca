"""debig_png_decode_batch_labels on the MI355X (include/decode_png.h; api.png_decode_batch_labels): the whole call BIT FOR BIT
against the numpy restatement (tests/png_label_ref.py) -- every colour type, depth, interlace and tRNS combination and
palette files of other sizes in ONE batch, all four dtypes, with and without a LUT; against the calls that already exist
(the nearest filter of png_decode_batch_tensor, png_decode_batch); per-image boxes; E_LABEL / E_BOX and their order; bad files
in the middle of a batch with a sentinel-filled tensor; nothing outside the tensor written; a real palette file."""
import ctypes as C
import glob
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_ref as LR  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_gpu_png_spec as G  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ["uint8", "uint16", "int32", "int64"]
RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resources")
LUT = np.random.default_rng(99).permutation(256).astype(np.int32)


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


def _palette_file(rng, w, h, n_pal, depth=8, il=0):
    pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(n_pal)]
    return R.encode(R.random_image(rng, w, h, 3, depth, n_pal), 3, depth, il, palette=pal, filters=lambda p, y: y % 5)


@pytest.fixture(scope="module")
def datas():
    """every file of _all_formats() (45 x 70: every colour type, depth, interlace, tRNS) and palette files of other sizes and
    palette lengths, interleaved"""
    rng = np.random.default_rng(78)
    fs = [d for _, d in G._all_formats()]
    pal = [_palette_file(rng, 1, 1, 2, 1), _palette_file(rng, 64, 65, 16, 4), _palette_file(rng, 333, 129, 21, 8, 1),
           _palette_file(rng, 5, 300, 256, 8)]
    out = []
    for k, f in enumerate(fs):
        out.append(f)
        if k % 9 == 0 and pal:
            out.append(pal.pop())
    return out + pal


_REF = {}


def _ref(data):
    """the restatement's raw labels of a file, computed once (dtype int64, no lut: E_LABEL by colour type alone)"""
    if data not in _REF:
        _REF[data] = LR.labels(data)
    return _REF[data]


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _check(api, datas, size, dtype, lut=None, boxes=None, fill=None, expect=None):
    st, t, infos = api.png_decode_batch_labels(datas, size, dtype=dtype, boxes=boxes, lut=lut, fill=fill)
    got = _np(t)
    assert got.shape == (len(datas),) + tuple(size) and got.dtype == LR.DTYPES[dtype]
    for i, data in enumerate(datas):
        rst, lab, inf = _ref(data)
        box = boxes[i] if boxes is not None else None
        want = rst
        if inf["width"] and LR.label_error(inf, dtype, lut):
            want = LR.E_LABEL
        elif inf["width"] and LR.box_error(box, inf["width"], inf["height"]):
            want = LR.E_BOX
        if expect is not None:
            assert want == expect[i], (i, want, expect[i])
        assert st[i] == want, (i, inf, st[i], want)
        if rst == 0:
            assert infos[i] == inf, i
        elif inf["width"]:
            assert infos[i]["color_type"] == inf["color_type"] and infos[i]["width"] == inf["width"], i
        if st[i] != 0:
            if fill is not None:
                assert (got[i] == np.array(fill).astype(got.dtype)).all(), (i, "a failed file's slot was written")
            continue
        exp = LR.gather(lab, size, box, lut, dtype)
        assert got[i].tobytes() == exp.tobytes(), (i, inf, size, dtype, box, np.argwhere(got[i] != exp)[:4])
    return st


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_lut", [False, True])
def test_mixed_batch_every_dtype_with_and_without_a_lut(api, datas, dtype, with_lut):
    """shrinking to (32, 24) and enlarging to (75, 50); colour types 2, 4, 6: E_LABEL; 16-bit grey: E_LABEL for uint8 and
    with a LUT; everything else bit for bit"""
    lut = LUT if with_lut else None
    for size in ((32, 24), (75, 50)):
        st = _check(api, datas, size, dtype, lut)
        for data, s in zip(datas, st):
            inf = _ref(data)[2]
            if inf["color_type"] in (2, 4, 6):
                assert s == LR.E_LABEL
            elif inf["bit_depth"] == 16:
                assert s == (LR.E_LABEL if dtype == "uint8" or with_lut else 0)
            else:
                assert s == 0


def test_against_the_nearest_filter_and_the_plain_decode(api, datas):
    """grey 8 without tRNS, and palette 8 whose PLTE entry i is (i, i, i): the uint8 labels are the bytes of
    png_decode_batch_tensor(mode="gray", dtype="uint", filter="nearest") with the same boxes; with size == (h, w) and no
    box the result is labels() itself"""
    rng = np.random.default_rng(5)
    grey_pal = [(i, i, i) for i in range(256)]
    files = [R.encode(R.random_image(rng, w, h, 0, 8), 0, 8, il, filters=lambda p, y: y % 5)
             for w, h, il in ((45, 70, 0), (45, 70, 1), (333, 129, 0), (1, 1, 0))]
    files += [R.encode(R.random_image(rng, w, h, 3, 8), 3, 8, il, palette=grey_pal, filters=lambda p, y: y % 5)
              for w, h, il in ((45, 70, 1), (64, 65, 0), (5, 300, 0))]
    boxes = [None, (3, 5, 40, 60), (100, 0, 233, 129), None, (44, 0, 1, 70), (0, 64, 64, 1), (0, 0, 0, 0)]
    for size in ((32, 24), (75, 50), (13, 100)):
        for bx in (None, boxes):
            st, t, _ = api.png_decode_batch_labels(files, size, dtype="uint8", boxes=bx)
            st2, t2, _ = api.png_decode_batch_tensor(files, size, mode="gray", depth=8, dtype="uint", layout="hwc", boxes=bx,
                                                     filter="nearest")
            assert st == st2 == [0] * len(files)
            assert _np(t).tobytes() == _np(t2).tobytes(), size
    for data in files + [d for d in datas if _ref(d)[0] == 0][:12]:
        _, lab, inf = _ref(data)
        for dtype in ("uint16", "int64"):
            st, t, _ = api.png_decode_batch_labels([data], (inf["height"], inf["width"]), dtype=dtype)
            assert st == [0] and np.array_equal(_np(t)[0], lab.astype(LR.DTYPES[dtype]))


def test_per_image_boxes_and_box_errors(api, datas):
    boxes = []
    for i, data in enumerate(datas):
        _, inf = api.png_info(data)
        w, h = inf["width"], inf["height"]
        k = i % 6
        boxes.append([None, (0, 0, 0, 0), (0, 0, max(w // 2, 1), max(h // 3, 1)), (w - max(w // 3, 1), h - max(h // 2, 1), max(w // 3, 1), max(h // 2, 1)),
                      (w - 1, 0, 1, h), (0, h - 1, w, 1)][k])
    for dtype, lut in (("int64", LUT), ("uint16", None), ("uint8", None)):
        _check(api, datas, (20, 16), dtype, lut, boxes=boxes)
    # box errors, and E_LABEL before E_BOX on an RGB file with a bad box
    rng = np.random.default_rng(3)
    rgb = R.encode(R.random_image(rng, 45, 70, 2, 8), 2, 8)
    g4 = R.encode(R.random_image(rng, 45, 70, 0, 4), 0, 4, 1)
    pal = _palette_file(rng, 45, 70, 7, 4)
    files = [g4, g4, pal, pal, rgb, g4, pal[:60], g4]
    bxs = [None, (40, 0, 6, 5), (0, 0, 0, 9), (5, 6, 7, 8), (0, 0, 46, 1), (0, 70, 1, 1), (0, 0, 46, 1), (0, 69, 45, 1)]
    B, Lb = LR.E_BOX, LR.E_LABEL
    st = _check(api, files, (3, 9), "int32", boxes=bxs, fill=-9, expect=[0, B, B, 0, Lb, B, B, 0])
    assert st == [0, B, B, 0, Lb, B, B, 0]


def _label_error_files():
    """the damage of test_gpu_png_spec._error_files() done to label files (8-bit grey, 4-bit palette), so that every status of
    the decode is reached behind E_LABEL"""
    rng = np.random.default_rng(6)
    s = R.random_image(rng, 20, 11, 0, 8)
    raw = R.scanlines(s, 0, 8)
    z = zlib.compress(raw)
    crc = bytearray(R.encode(s, 0, 8, zdata=z))
    crc[50] ^= 0x10
    p = R.random_image(rng, 20, 11, 3, 4, 9)
    pal = [(k, k, 9) for k in range(9)]
    pz = zlib.compress(R.scanlines(p, 3, 4))
    fl = 0x20 | ((31 - ((0x78 << 8) | 0x20) % 31) % 31)
    cases = [("crc", bytes(crc), R.E_CRC),
             ("adler wrong", R.encode(s, 0, 8, zdata=z[:-4] + bytes(4)), R.E_ADLER),
             ("adler missing", R.encode(p, 3, 4, palette=pal, zdata=pz[:-4]), R.E_ADLER),
             ("short data", R.encode(s, 0, 8, zdata=zlib.compress(raw[:-5])), R.E_DATA_SHORT),
             ("long data", R.encode(p, 3, 4, palette=pal, zdata=zlib.compress(R.scanlines(p, 3, 4) + bytes(9))), R.E_DATA_LONG),
             ("inflate", R.encode(s, 0, 8, zdata=z[:2] + bytes([0x01, 5, 0, 0, 0]) + z[7:]), R.E_INFLATE),
             ("filter 5", R.encode(s, 0, 8, filters=lambda q, y: 5 if y == 7 else 1), R.E_FILTER),
             ("fdict", R.encode(s, 0, 8, zdata=bytes([0x78, fl]) + b"\0\0\0\1" + z[2:]), R.E_ZLIB),
             ("no plte", R.encode(p, 3, 4), R.E_CHUNK)]
    for name, data, st in cases:
        assert R.decode(data)[0] == st, name
    return cases


def test_bad_files_in_the_middle_of_a_batch_leave_their_slots(api, datas):
    """the files of test_gpu_png_spec._error_files() -- colour type 6 is E_LABEL at IHDR, the others keep their status --, the
    same damage on label files, b"not a png" and a truncated file: statuses as png_decode_batch gives them, slots untouched"""
    cases = G._error_files() + _label_error_files()
    good = [d for d in datas if _ref(d)[0] == 0][:4]
    batch = good[:2] + [d for _, d, _ in cases] + [b"not a png", good[3][:40]] + good[2:]
    plain = [s for s, _, _ in api.png_decode_batch(batch)]
    names = [n for n, _, _ in cases]
    for dtype, fill in (("int64", -77), ("uint8", 0xA5), ("uint16", 0xBEEF)):
        st = _check(api, batch, (19, 21), dtype, fill=fill)
        for k, (data, s, p) in enumerate(zip(batch, st, plain)):
            inf = _ref(data)[2]
            if inf["width"] and inf["color_type"] not in (0, 3):
                assert s == LR.E_LABEL, k  # decided at IHDR, before the damage is found
            else:
                assert s == p, (k, s, p)
        for k, (name, _, want) in enumerate(cases):
            if k >= len(G._error_files()) or name in ("palette index", "palette index 2-bit", "filter 5 interlaced"):
                assert st[2 + k] == want, name
        for n in ("palette index", "palette index 2-bit"):
            assert st[2 + names.index(n)] == R.E_PALETTE
        assert st[:2] == [0, 0] and st[-2:] == [0, 0] and st[-4:-2] == [R.E_SIGNATURE, R.E_CHUNK]


def test_nothing_outside_the_tensor_is_written(api, datas):
    """the C call on a slice in the middle of a sentinel-filled allocation"""
    import torch
    from debigulator_amd import _native as N

    L = api._png_spec_lib()
    L.debig_png_decode_batch_labels.restype = C.c_int
    L.debig_png_decode_batch_labels.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p]
    ok = [d for d in datas if _ref(d)[0] == 0 and _ref(d)[2]["bit_depth"] < 16]
    files = ok[:5] + [b"not a png"] + ok[5:10]
    n = len(files)
    ins = [np.frombuffer(f, np.uint8) for f in files]
    for dtype, size in (("int64", (13, 100)), ("uint8", (33, 31)), ("int64", (33, 31)), ("uint8", (13, 100))):
        d, es = api.png_label_desc(size, dtype, LUT if dtype == "int64" else None)
        slot = size[0] * size[1] * es
        arena = torch.full((4096 + n * slot + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        st = (C.c_uint32 * n)()
        rc = L.debig_png_decode_batch_labels((C.c_void_p * n)(*[a.ctypes.data for a in ins]), (C.c_uint64 * n)(*[len(f) for f in files]),
                                             arena.data_ptr() + 4096, None, st, None, n, 0, C.byref(d))
        N.check(rc, "debig_png_decode_batch_labels")
        a = arena.cpu().numpy()
        assert list(st) == [0] * 5 + [R.E_SIGNATURE] + [0] * 5
        assert (a[:4096] == 0xA5).all() and (a[4096 + n * slot:] == 0xA5).all() and (a[4096 + 5 * slot: 4096 + 6 * slot] == 0xA5).all()
        for i in (0, 4, 6, 10):
            want = LR.gather(_ref(files[i])[1], size, None, LUT if dtype == "int64" else None, dtype)
            assert a[4096 + i * slot: 4096 + (i + 1) * slot].tobytes() == want.tobytes(), (dtype, size, i)


def test_trns_and_plte_colours_do_not_change_the_labels(api):
    rng = np.random.default_rng(12)
    outs = []
    for depth, n_pal in ((8, 200), (4, 16), (2, 3)):
        s = R.random_image(rng, 61, 37, 3, depth, n_pal)
        pal_a = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(n_pal)]
        pal_b = [(0, 0, 0)] * n_pal
        files = [R.encode(s, 3, depth, 0, palette=pal_a), R.encode(s, 3, depth, 1, palette=pal_b),
                 R.encode(s, 3, depth, 0, palette=pal_a, trns=bytes(n_pal)), R.encode(s, 3, depth, 1, palette=pal_b, trns=b"\x07")]
        st, t, infos = api.png_decode_batch_labels(files, (37, 61), dtype="uint8")
        got = _np(t)
        assert st == [0] * 4 and [i["has_trns"] for i in infos] == [0, 0, 1, 1]
        for k in range(4):
            assert np.array_equal(got[k], s[:, :, 0])
        outs.append(got)
    g = R.random_image(rng, 61, 37, 0, 2)
    st, t, infos = api.png_decode_batch_labels([R.encode(g, 0, 2), R.encode(g, 0, 2, 1, trns=b"\x00\x02")], (37, 61), dtype="int32")
    assert st == [0, 0] and infos[1]["has_trns"] == 1 and np.array_equal(_np(t)[0], g[:, :, 0]) and np.array_equal(_np(t)[1], g[:, :, 0])


def test_a_real_palette_file(api):
    """the first colour-type-3 file of tests/golden/resources: its labels run through its own palette are
    png_decode_batch(mode="rgb")"""
    paths = sorted(glob.glob(os.path.join(RES, "*.png")))
    data = next(d for d in (open(p, "rb").read() for p in paths) if api.png_info(d)[1]["color_type"] == 3)
    inf = api.png_info(data)[1]
    st, t, _ = api.png_decode_batch_labels([data], (inf["height"], inf["width"]), dtype="int64")
    hst, rgb, _ = api.png_decode_batch([data], mode="rgb")[0]
    assert st == [0] and hst == 0
    pal = R._walk(data)[2][0]
    lab = _np(t)[0]
    assert lab.max() < len(pal) and np.array_equal(pal[lab][:, :, :3], rgb)
    assert np.array_equal(lab, _ref(data)[1])
    # and through a LUT, shrunk: the restatement
    _check(api, [data], (48, 40), "int32", LUT)
