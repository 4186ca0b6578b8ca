"""debig_png_decode_batch_layout / debig_png_decode_batch_dev (include/decode_png.h) without a GPU: the argument checks
that come before any file is looked at and before any device work, the Python layout argument, the exported symbols."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BAD_FORMAT, BAD_ARG = -1, -2
DUMMY = 0x10000  # a non-NULL address that is never dereferenced: the calls below return before any device work


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_decode_batch_layout.restype = C.c_int
    L.debig_png_decode_batch_layout.argtypes = [C.c_void_p] * 6 + [C.c_uint32] * 4
    L.debig_png_decode_batch_dev.restype = C.c_int
    L.debig_png_decode_batch_dev.argtypes = [C.c_void_p] * 7 + [C.c_uint32] * 4
    return L


def _inputs(n):
    bufs = [C.create_string_buffer(b"not a png", 9) for _ in range(n)]
    return bufs, (C.c_void_p * n)(*[C.addressof(b) for b in bufs]), (C.c_uint64 * n)(*[9] * n)


def _dev(lib, arena, offs, caps, fmt=0, layout=0):
    n = len(offs)
    bufs, ins, sizes = _inputs(n)
    st = (C.c_uint32 * n)(*[0xABCD] * n)
    rc = lib.debig_png_decode_batch_dev(ins, sizes, arena, (C.c_uint64 * n)(*offs), (C.c_uint64 * n)(*caps), st, None, n, 0,
                                        fmt, layout)
    return rc, list(st)


@pytest.mark.parametrize("layout", [2, 3, 0x10, 0x80000000, 0xFFFFFFFF])
def test_bad_layout_is_bad_format_from_both_calls(lib, layout):
    bufs, ins, sizes = _inputs(1)
    out = C.create_string_buffer(64)
    st = (C.c_uint32 * 1)(0xABCD)
    rc = lib.debig_png_decode_batch_layout(ins, sizes, (C.c_void_p * 1)(C.addressof(out)), (C.c_uint64 * 1)(64), st, None, 1, 0,
                                           0, layout)
    assert rc == BAD_FORMAT and st[0] == 0xABCD and out.raw == bytes(64)
    rc, st = _dev(lib, DUMMY, [0], [64], 0, layout)
    assert rc == BAD_FORMAT and st == [0xABCD]


@pytest.mark.parametrize("fmt", [5, 0x30, 0x40, 0x100])
def test_bad_format_from_both_calls(lib, fmt):
    bufs, ins, sizes = _inputs(1)
    out = C.create_string_buffer(64)
    st = (C.c_uint32 * 1)(0xABCD)
    for layout in (0, 1):
        rc = lib.debig_png_decode_batch_layout(ins, sizes, (C.c_void_p * 1)(C.addressof(out)), (C.c_uint64 * 1)(64), st, None,
                                               1, 0, fmt, layout)
        assert rc == BAD_FORMAT and st[0] == 0xABCD
        rc, sd = _dev(lib, DUMMY, [0], [64], fmt, layout)
        assert rc == BAD_FORMAT and sd == [0xABCD]


@pytest.mark.parametrize("off", [1, 4, 8, 15, 17, 4096 + 8])
def test_misaligned_offset_is_bad_arg(lib, off):
    for layout in (0, 1):
        rc, st = _dev(lib, DUMMY, [0, off, 8192], [16, 16, 16], 0, layout)
        assert rc == BAD_ARG and st == [0xABCD] * 3


def test_null_arena_is_bad_arg(lib):
    rc, st = _dev(lib, None, [0, 64], [64, 64])
    assert rc == BAD_ARG and st == [0xABCD] * 2
    bufs, ins, sizes = _inputs(1)
    assert lib.debig_png_decode_batch_dev(ins, sizes, None, None, None, None, None, 0, 0, 0, 0) == 0  # n == 0: nothing to do


@pytest.mark.parametrize("offs,caps", [([0, 16], [17, 16]), ([0, 0], [16, 16]), ([64, 0, 128], [16, 80, 16]),
                                       ([256, 0], [16, 1024]), ([0, 32, 16], [16, 16, 32]),
                                       ([16, 2 ** 64 - 16], [16, 32])])
def test_overlapping_regions_are_bad_arg(lib, offs, caps):
    rc, st = _dev(lib, DUMMY, offs, caps)
    assert rc == BAD_ARG and st == [0xABCD] * len(offs)


def test_good_arguments_reach_the_files(lib):
    """adjacent regions, empty regions at one offset: accepted; the files then fail on the host (no device work)"""
    rc, st = _dev(lib, DUMMY, [0, 16, 32, 32, 48], [16, 16, 0, 0, 16], 0, 1)
    assert rc == 0 and st == [1] * 5  # DEBIG_PNG_E_SIGNATURE
    bufs, ins, sizes = _inputs(2)
    outs = [C.create_string_buffer(64) for _ in range(2)]
    st = (C.c_uint32 * 2)()
    rc = lib.debig_png_decode_batch_layout(ins, sizes, (C.c_void_p * 2)(*[C.addressof(o) for o in outs]),
                                           (C.c_uint64 * 2)(64, 64), st, None, 2, 0, 0x11, 1)
    assert rc == 0 and list(st) == [1, 1]


def test_python_layout_argument():
    from debigulator_amd import api

    with pytest.raises(ValueError):
        api.png_decode_batch([b"x"], layout="bogus")
    with pytest.raises(ValueError):
        api.png_decode_batch_device([b"x"], layout="planar")
    with pytest.raises(ValueError):
        api.png_decode_batch_device([b"x"], mode="bgr")
    assert api.png_layout_code("hwc") == 0 and api.png_layout_code("chw") == 1


def test_symbols_are_exported(lib):
    from debigulator_amd import _native as N

    out = os.popen(f"nm -D --defined-only {N.LIB_PATH}").read()
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"debig_png_decode_batch_layout", "debig_png_decode_batch_dev", "debig_hip_png_spec_defilter_planar_batch",
            "debig_png_decode_batch_fmt"} <= syms
