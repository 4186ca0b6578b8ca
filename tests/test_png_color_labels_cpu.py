"""debig_png_decode_batch_color_labels without a GPU (include/decode_png.h): the numpy restatement
tests/png_color_label_ref.py against the reference decoder the rest of the suite uses, the host's table builder
(debig_png_color_map_table) against the restated slot rule, and what the C call decides on the host alone: every argument
check (status and unmatched left at their sentinels) and the statuses E_LABEL / E_BOX, their order included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_label_ref as CR  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_gpu_png_spec as G  # noqa: E402

BAD_ARG = -2
DUMMY = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced: the calls below never reach the device
U8, U16, I32, I64 = range(4)
PACK, MAP = 0, 1
SENTINEL = 0xABCD


class ColorMap(C.Structure):  # include/decode_png.h: debig_png_color_map
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32), ("keys", C.POINTER(C.c_uint32)), ("values", C.POINTER(C.c_int32))]


class ColorLabelDesc(C.Structure):  # include/decode_png.h: debig_png_color_label_desc
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("dtype", C.c_uint32), ("mode", C.c_uint32), ("missing", C.c_int32),
                ("n_maps", C.c_uint32), ("maps", C.POINTER(ColorMap)), ("reserved", C.c_uint32), ("reserved2", C.c_uint32)]


class Box(C.Structure):  # include/decode_png.h: debig_png_box
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_decode_batch_color_labels.restype = C.c_int
    L.debig_png_decode_batch_color_labels.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p]
    L.debig_png_color_map_table.restype = C.c_uint32
    L.debig_png_color_map_table.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    return L


def _map(keys, values=None, n=None, null_keys=False, null_values=False):
    keys = list(keys)
    values = list(range(len(keys))) if values is None else list(values)
    m = ColorMap(n=len(keys) if n is None else n)
    m._keep = ((C.c_uint32 * max(len(keys), 1))(*keys), (C.c_int32 * max(len(values), 1))(*values))
    if not null_keys:
        m.keys = C.cast(m._keep[0], C.POINTER(C.c_uint32))
    if not null_values:
        m.values = C.cast(m._keep[1], C.POINTER(C.c_int32))
    return m


# ---- the restatement against the rest of the suite --------------------------------------------------------------------------

def test_rgb_of_the_restatement_against_the_reference_decoder():
    """8-bit RGB / RGBA, grey 8 and palette files: the colours are the first three channels of R.decode's RGBA8; sub-byte grey
    is scaled by 255 / 85 / 17; 16-bit files of every colour type: E_LABEL"""
    seen = set()
    for (ct, depth, il, trns), data in G._all_formats():
        st, px, inf = CR.rgb(data)
        est, rgba, einf = R.decode(data)
        assert est == R.OK and inf == einf
        if depth == 16:
            assert st == CR.E_LABEL and px is None
            continue
        assert st == R.OK and px.shape == (70, 45, 3) and px.dtype == np.uint8
        assert np.array_equal(px, rgba[:, :, :3]), (ct, depth, il, trns)
        if ct == 0 and depth < 8:
            assert set(np.unique(px)) <= {v * {1: 255, 2: 85, 4: 17}[depth] for v in range(1 << depth)}
        seen.add((ct, depth))
    assert seen == {(ct, d) for ct in R.DEPTHS for d in R.DEPTHS[ct] if d != 16}


def test_gather_restatement_on_a_small_case():
    px = np.zeros((2, 3, 3), np.uint8)
    px[..., 0] = [[1, 2, 3], [4, 5, 6]]
    px[..., 1] = 7
    px[1, 2] = (255, 255, 255)
    key = CR.pack(px)
    assert key.tolist() == [[0x0701, 0x0702, 0x0703], [0x0704, 0x0705, 0xFFFFFF]]
    assert CR.gather(px, (2, 3), dtype="int32")[0].tolist() == key.tolist()
    out, miss = CR.gather(px, (1, 2), None, {0x0704: -4, 0xFFFFFF: 9}, -1, "int64")
    assert out.tolist() == [[-4, 9]] and miss == 0
    out, miss = CR.gather(px, (2, 6), (1, 0, 2, 2), {0x0702: 2}, 255, "uint8")
    assert out.tolist() == [[2, 2, 2, 255, 255, 255], [255] * 6] and miss == 9


# ---- the host's table builder -------------------------------------------------------------------------------------------------

def _host_table(lib, m, cap=4096):
    t = np.full((cap, 2), 0x5A5A5A5A, dtype=np.uint32)
    slots = lib.debig_png_color_map_table(C.byref(m), t.ctypes.data, cap)
    assert (t[slots:] == 0x5A5A5A5A).all()
    return slots, t[:slots]


def test_table_builder_against_the_restated_slot_rule(lib):
    rng = np.random.default_rng(17)
    for n in (0, 1, 2, 3, 64, 65, 1000, 1024, 1025, 2048):
        keys = [int(k) for k in rng.choice(1 << 24, size=n, replace=False)]
        if n >= 2:
            keys[0], keys[1] = 0x000000, 0xFFFFFF
            keys = list(dict.fromkeys(keys))
            n = len(keys)
        values = [int(v) for v in rng.integers(-2 ** 31, 2 ** 31, n)]
        slots, t = _host_table(lib, _map(keys, values))
        assert slots == CR.slots_for(n) and slots >= 2 * n and slots >= 2 and slots & (slots - 1) == 0
        assert np.array_equal(t, CR.table(keys, values)), n
        assert int((t[:, 0] != CR.EMPTY).sum()) == n
    # keys that share a slot sit behind one another in insertion order, wrapping at the end of the table
    k = np.arange(1 << 24, dtype=np.uint64)
    same = [int(v) for v in k[((((k * 0x9E3779B1) & 0xFFFFFFFF) >> 20) & 127) == 126][:64]]
    slots, t = _host_table(lib, _map(same))
    assert slots == 128 and [int(v) for v in t[(126 + np.arange(64)) % 128, 0]] == same
    assert np.array_equal(t, CR.table(same, range(64)))


def test_table_builder_refuses_what_the_call_refuses(lib):
    t = np.zeros((4096, 2), dtype=np.uint32)
    for m in (_map(range(2049)), _map([1, 2], null_keys=True), _map([1, 2], null_values=True), _map([1, 0x1000000]),
              _map([5, 6, 5]), _map([0xFFFFFFFF])):
        assert lib.debig_png_color_map_table(C.byref(m), t.ctypes.data, 4096) == 0
        assert not t.any()
    assert lib.debig_png_color_map_table(None, t.ctypes.data, 4096) == 0
    assert lib.debig_png_color_map_table(C.byref(_map(range(5))), t.ctypes.data, 8) == 0  # needs 16 slots
    assert lib.debig_png_color_map_table(C.byref(_map(range(5))), t.ctypes.data, 16) == 16
    assert lib.debig_png_color_map_table(C.byref(_map([], n=0, null_keys=True, null_values=True)), t.ctypes.data, 2) == 2


# ---- the C call: what needs no device -----------------------------------------------------------------------------------------

def _desc(out_w=8, out_h=6, dtype=I64, mode=PACK, missing=-1, maps=None, n_maps=None, reserved=0, null_maps=False):
    d = ColorLabelDesc(out_w=out_w, out_h=out_h, dtype=dtype, mode=mode, missing=missing, reserved=reserved)
    if maps is not None:
        d._keep = (ColorMap * len(maps))(*maps)
        d._maps = maps
        if not null_maps:
            d.maps = C.cast(d._keep, C.POINTER(ColorMap))
    d.n_maps = (len(maps) if maps is not None else 0) if n_maps is None else n_maps
    return d


def _call(lib, files, desc, out=DUMMY, boxes=None):
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    st = (C.c_uint32 * n)(*[SENTINEL] * n)
    um = (C.c_uint32 * n)(*[SENTINEL] * n)
    bx = (Box * n)(*[Box(*b) if b else Box(0, 0, 0, 0) for b in boxes]) if boxes else None
    rc = lib.debig_png_decode_batch_color_labels(ins, sizes, out, bx, st, None, um, n, 0, C.byref(desc) if desc is not None else None)
    return rc, list(st), list(um)


def bad_arg_cases(n=2):
    """(name, desc, d_out offset) of every DEBIG_PNG_BAD_ARG rule, for a batch of n files (also used by the GPU test)"""
    one = [_map([1, 2, 3])]
    return [("desc NULL", None, 0), ("d_out NULL", _desc(), None), ("d_out unaligned", _desc(), 8),
            ("out_w 0", _desc(out_w=0), 0), ("out_w 16385", _desc(out_w=16385), 0), ("out_h 0", _desc(out_h=0), 0),
            ("out_h 16385", _desc(out_h=16385), 0), ("dtype", _desc(dtype=4), 0), ("reserved", _desc(reserved=1), 0),
            ("mode", _desc(mode=2, maps=one), 0), ("pack u8", _desc(dtype=U8), 0), ("pack u16", _desc(dtype=U16), 0),
            ("pack with maps", _desc(maps=one), 0), ("pack n_maps", _desc(n_maps=1), 0),
            ("map n_maps 0", _desc(mode=MAP, maps=one, n_maps=0), 0), ("map n_maps n + 1", _desc(mode=MAP, maps=one * (n + 1)), 0),
            ("map n_maps between", _desc(mode=MAP, maps=one * (n + 1), n_maps=n - 1 if n > 2 else n + 1), 0),
            ("maps NULL", _desc(mode=MAP, maps=one, null_maps=True), 0),
            ("map too large", _desc(mode=MAP, maps=[_map(range(2049))]), 0),
            ("keys NULL", _desc(mode=MAP, maps=[_map([1], null_keys=True)]), 0),
            ("values NULL", _desc(mode=MAP, maps=[_map([1], null_values=True)]), 0),
            ("key above 24 bits", _desc(mode=MAP, maps=[_map([1, 0x1000000])]), 0),
            ("equal keys", _desc(mode=MAP, maps=[_map([7, 8, 9, 7])]), 0),
            ("equal keys in the last of n maps", _desc(mode=MAP, maps=one * (n - 1) + [_map([4, 4])]), 0),
            ("u8 value 256", _desc(dtype=U8, mode=MAP, missing=0, maps=[_map([1, 2], [0, 256])]), 0),
            ("u8 value -1", _desc(dtype=U8, mode=MAP, missing=0, maps=[_map([1, 2], [-1, 0])]), 0),
            ("u8 missing -1", _desc(dtype=U8, mode=MAP, missing=-1, maps=one), 0),
            ("u8 missing 256", _desc(dtype=U8, mode=MAP, missing=256, maps=one), 0),
            ("u16 value 65536", _desc(dtype=U16, mode=MAP, missing=0, maps=[_map([1], [65536])]), 0),
            ("u16 missing -1", _desc(dtype=U16, mode=MAP, missing=-1, maps=one), 0)]


def test_argument_checks_leave_status_and_unmatched_unwritten(lib):
    for name, desc, off in bad_arg_cases(2):
        out = None if off is None else DUMMY + off
        assert _call(lib, [b"not a png", b"x"], desc, out) == (BAD_ARG, [SENTINEL] * 2, [SENTINEL] * 2), name
    # n == 0: nothing is checked, nothing is done
    assert lib.debig_png_decode_batch_color_labels(None, None, None, None, None, None, None, 0, 0, None) == 0
    # the same arguments at the edge of their ranges pass the checks and reach the files
    ok = [_desc(out_w=16384, out_h=16384), _desc(dtype=I32), _desc(mode=MAP, maps=[_map([])]),
          _desc(mode=MAP, maps=[_map([], n=0, null_keys=True, null_values=True)] * 2),
          _desc(mode=MAP, maps=[_map(range(2048))]), _desc(mode=MAP, maps=[_map([0, 0xFFFFFF], [-2 ** 31, 2 ** 31 - 1])], missing=-2 ** 31),
          _desc(dtype=U8, mode=MAP, missing=255, maps=[_map([1, 2], [0, 255])]),
          _desc(dtype=U16, mode=MAP, missing=65535, maps=[_map([1, 2], [0, 65535]), _map([2, 1])]),
          _desc(dtype=I32, missing=-77)]  # (PACK does not read `missing`)
    for desc in ok:
        assert _call(lib, [b"not a png", b"x"], desc) == (0, [R.E_SIGNATURE] * 2, [0, 0])
    assert _call(lib, [b"not a png"], _desc(), DUMMY + 16) == (0, [R.E_SIGNATURE], [0])


def test_label_and_box_statuses_are_decided_on_the_host(lib):
    """E_LABEL iff the file is 16-bit, then E_BOX, as soon as IHDR has been read: both outrank what the file holds later (here
    a damaged CRC and a missing IDAT), and the walk's own statuses before IHDR come first"""
    rng = np.random.default_rng(4)
    rgb16 = R.encode(R.random_image(rng, 9, 7, 2, 16), 2, 16)
    ga16 = R.encode(R.random_image(rng, 9, 7, 4, 16), 4, 16)
    rgba16 = R.encode(R.random_image(rng, 9, 7, 6, 16), 6, 16)
    g16 = R.encode(R.random_image(rng, 9, 7, 0, 16), 0, 16)
    rgb = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    pal = R.encode(R.random_image(rng, 9, 7, 3, 4, 5), 3, 4, palette=[(1, 2, 3)] * 5)
    rgb_crc = bytearray(rgb)
    rgb_crc[-20] ^= 1
    files = [rgb16, ga16, rgba16, g16, rgb, pal, rgb[:40], bytes(rgb_crc), rgb[:33], b"\x89PNG"]
    boxes = [None, None, (0, 0, 10, 1), (0, 0, 10, 1), (0, 0, 10, 1), (3, 3, 0, 2), (8, 6, 2, 1), (0, 7, 9, 1), None, None]
    L, B = CR.E_LABEL, CR.E_BOX
    want = [L, L, L, L, B, B, B, B, R.E_CHUNK, R.E_SIGNATURE]
    for desc in (_desc(), _desc(dtype=U8, mode=MAP, missing=0, maps=[_map([1, 2])])):
        assert _call(lib, files, desc, boxes=boxes) == (0, want, [0] * len(files))
    for data in files[:4]:
        assert CR.rgb(data)[0] == L


def test_python_descriptor(lib):
    from debigulator_amd import api

    d, es = api.png_color_label_desc((6, 8), None, dtype="int32")
    assert (d.out_w, d.out_h, d.dtype, d.mode, d.n_maps, d.reserved, es) == (8, 6, I32, PACK, 0, 0, 4) and not d.maps
    d, es = api.png_color_label_desc((6, 8), {(1, 2, 3): 5, (255, 255, 255): -1}, missing=-9, dtype="int64")
    assert (d.mode, d.missing, d.n_maps, es) == (MAP, -9, 1, 8)
    assert [d.maps[0].keys[k] for k in range(2)] == [0x030201, 0xFFFFFF] and [d.maps[0].values[k] for k in range(2)] == [5, -1]
    d, _ = api.png_color_label_desc((1, 1), [({}), (np.array([[0, 0, 1]]), np.array([3])), ([7, 8], [1, 2])], dtype="uint8", n=3)
    assert d.n_maps == 3 and [d.maps[k].n for k in range(3)] == [0, 1, 2] and d.maps[1].keys[0] == 0x010000 and d.maps[2].keys[1] == 8
    assert api.png_pack_rgb([[1, 2, 3]]).tolist() == [0x030201]
    # the ctypes mirrors are the C structs: the C call reads what Python wrote
    assert _call(lib, [b"not a png"], d)[0] == BAD_ARG  # three maps for one file
    assert _call(lib, [b"a", b"b", b"c"], d) == (BAD_ARG, [SENTINEL] * 3, [SENTINEL] * 3)  # missing = -1 with uint8
    d, _ = api.png_color_label_desc((1, 1), [({}), (np.array([[0, 0, 1]]), np.array([3])), ([7, 8], [1, 2])], 0, "uint8", n=3)
    assert _call(lib, [b"a", b"b", b"c"], d) == (0, [R.E_SIGNATURE] * 3, [0] * 3)
    for kw in (dict(size=(0, 4)), dict(size=(4, 16385)), dict(size=(4, 4), dtype="float32"), dict(size=(4, 4), dtype="uint8"),
               dict(size=(4, 4), colors=[{}], n=2), dict(size=(4, 4), colors={(1, 2, 256): 0}), dict(size=(4, 4), colors=([1, 2], [1])),
               dict(size=(4, 4), colors="red"), dict(size=(4, 4), colors={(1, 2, 3): 0}, missing=2 ** 31)):
        with pytest.raises(ValueError):
            api.png_color_label_desc(**kw)
