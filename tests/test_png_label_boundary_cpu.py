"""The label boundary without a GPU (include/decode_png.h: debig_png_label_boundary): the numpy restatement
tests/png_label_boundary_ref.py on a map worked out by hand and against scipy's min / max filters, the host's reach tables against
the restatement, every argument check of the C call that is decided before a device is touched, the argument rules of
png_label_boundary, the unchanged signatures of the two label decode calls, the new symbols, and the stand-alone sanitizer program of
the kernel on the emulator."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_boundary_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -2
DUMMY = 0x10000  # "device pointers" that are never followed: every case below is refused before a device is touched
SQUARE, DIAMOND, DISK, RING, EDGE = 0, 1, 2, 0, 1


@pytest.fixture(scope="module")
def api():
    from debigulator_amd import api as A_

    return A_


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_label_boundary_reach.restype = None
    L.debig_png_label_boundary_reach.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    L.debig_png_label_boundary.restype = C.c_int
    L.debig_png_label_boundary.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_int64, C.c_void_p]
    return L


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def test_the_restatement_on_a_map_worked_out_by_hand():
    img = np.array([[1, 1, 1, 1, 1],
                    [1, 1, 1, 1, 1],
                    [1, 1, 2, 1, 1],
                    [1, 1, 1, 1, 1]], np.int32)
    assert R.reach(1, "square") == [1, 1] and R.reach(1, "diamond") == [1, 0] and R.reach(1, "disk") == [1, 0]
    sq = R.boundary(img, R.reach(1, "square")).astype(int)
    assert sq.tolist() == [[0, 0, 0, 0, 0],
                           [0, 1, 1, 1, 0],
                           [0, 1, 1, 1, 0],
                           [0, 1, 1, 1, 0]]  # 8-connected; the lone element itself is marked: the rule is symmetric
    di = R.boundary(img, R.reach(1, "diamond")).astype(int)
    assert di.tolist() == [[0, 0, 0, 0, 0],
                           [0, 0, 1, 0, 0],
                           [0, 1, 1, 1, 0],
                           [0, 0, 1, 0, 0]]  # 4-connected
    assert R.reach(2, "diamond") == [2, 1, 0] and R.reach(2, "disk") == [2, 1, 0] and R.reach(3, "disk") == [3, 2, 2, 0]
    d2 = R.boundary(img, R.reach(2, "diamond")).astype(int)
    assert d2.tolist() == [[0, 0, 1, 0, 0],
                           [0, 1, 1, 1, 0],
                           [1, 1, 1, 1, 1],
                           [0, 1, 1, 1, 0]]  # clipped at the bottom, never padded
    ring = R.apply(img[None], 1, "diamond", "ring", 255)[0]
    assert ring.dtype == np.int32 and ring.tolist() == [[1, 1, 1, 1, 1], [1, 1, 255, 1, 1], [1, 255, 255, 255, 1], [1, 1, 255, 1, 1]]
    edge = R.apply(img[None], 1, "diamond", "edge")[0]
    assert edge.dtype == np.uint8 and np.array_equal(edge, di)
    # a flat image, a 1 x 1 image and an edge of the image make no boundary; a skipped image is the input / zeros
    assert not R.boundary(np.full((5, 7), 9), R.reach(16, "square")).any() and not R.boundary(np.array([[4]]), [3, 3, 3, 3]).any()
    both = np.stack([img, img])
    assert np.array_equal(R.apply(both, 1, "square", "ring", 7, status=[3, 0])[0], img)
    assert not R.apply(both, 1, "square", "edge", status=[3, 0])[0].any() and R.apply(both, 1, "square", "edge", status=[3, 0])[1].any()
    # elements are compared whole
    big = np.array([[3, 2 ** 32 + 3], [3, 3]], np.int64)
    assert R.boundary(big, [1, 0]).tolist() == [[True, True], [False, True]]
    assert R.apply(np.array([[[-1, 255]]], np.int32), 1, "square", "edge").tolist() == [[[1, 1]]]


def test_the_restatement_against_scipy_filters():
    """min != max over the clipped footprint: mode="nearest" repeats the edge element, which adds no new value to a window"""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for H, W in ((1, 1), (1, 7), (9, 1), (3, 4), (20, 33)):
        img = np.repeat(rng.integers(0, 4, (H, -(-W // 3))), 3, axis=1)[:, :W].astype(np.int64)
        for shape in R.SHAPES:
            for radius in (1, 2, 3, 5, 16):
                F = R.footprint(radius, shape)
                want = ndi.maximum_filter(img, footprint=F, mode="nearest") != ndi.minimum_filter(img, footprint=F, mode="nearest")
                assert np.array_equal(R.boundary(img, R.reach(radius, shape)), want), (H, W, shape, radius)


def test_the_restatement_against_brute_force():
    """(where scipy is absent: the rule element by element)"""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 3, (9, 11)).astype(np.int32)
    img[2:7, 3:9] = 1
    for shape in R.SHAPES:
        for radius in (1, 2, 5):
            table = R.reach(radius, shape)
            want = np.zeros(img.shape, bool)
            for y in range(9):
                for x in range(11):
                    for dy in range(-radius, radius + 1):
                        for dx in range(-table[abs(dy)], table[abs(dy)] + 1):
                            if 0 <= y + dy < 9 and 0 <= x + dx < 11 and img[y + dy, x + dx] != img[y, x]:
                                want[y, x] = True
            assert np.array_equal(R.boundary(img, table), want), (shape, radius)


# ---- the host's reach tables -------------------------------------------------------------------------------------------------------------

def test_host_reach_tables_against_the_restatement(lib, api):
    for shape, code in R.SHAPES.items():
        for radius in range(1, R.MAX_RADIUS + 1):
            table = (C.c_uint8 * 17)(*([0xEE] * 17))
            lib.debig_png_label_boundary_reach(radius, code, table)
            assert list(table) == R.reach(radius, shape) + [0] * (16 - radius), (shape, radius)
            assert api.png_label_boundary_reach(radius, shape) == R.reach(radius, shape)
            assert all(v * v + d * d <= radius * radius or shape != "disk" for d, v in enumerate(R.reach(radius, shape)))
    for radius, code in ((17, 0), (3, 3), (2 ** 32 - 1, 2)):
        table = (C.c_uint8 * 17)(*([0xEE] * 17))
        lib.debig_png_label_boundary_reach(radius, code, table)
        assert list(table) == [0] * 17
    assert api.png_label_boundary_reach(5, "disk") == [5, 4, 4, 4, 3, 0] and api.png_label_boundary_reach(2) == [2, 2, 2]
    for bad in (0, 17, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="radius"):
            api.png_label_boundary_reach(bad, "disk")
    for bad in ("circle", 0, None):
        with pytest.raises(ValueError, match="shape"):
            api.png_label_boundary_reach(3, bad)


# ---- the C call's argument checks --------------------------------------------------------------------------------------------------------

def test_c_argument_checks_come_before_any_device_work(lib):
    img = 33 * 24
    good = dict(d=DUMMY, o=DUMMY + 0x100000, n=2, w=33, h=24, dtype=3, r=2, shape=DISK, mode=RING, value=255, status=None)
    bad = [dict(d=None), dict(o=None), dict(d=DUMMY + 4), dict(o=DUMMY + 0x100004), dict(d=DUMMY + 1, dtype=1), dict(o=DUMMY + 0x100002, dtype=2),
           dict(r=0), dict(r=17), dict(r=2 ** 32 - 1), dict(shape=3), dict(shape=2 ** 31), dict(mode=2), dict(mode=2 ** 31), dict(dtype=4),
           dict(dtype=2 ** 31), dict(w=0), dict(w=16385), dict(h=0), dict(h=16385),
           dict(dtype=0, value=256), dict(dtype=0, value=-1), dict(dtype=1, value=65536), dict(dtype=1, value=-1),
           dict(dtype=2, value=2 ** 31), dict(dtype=2, value=-2 ** 31 - 1),
           dict(o=DUMMY), dict(o=DUMMY + 8), dict(o=DUMMY + 2 * img * 8 - 8), dict(d=DUMMY + 0x100000 + 2 * img * 8 - 8),
           dict(mode=EDGE, o=DUMMY + 2 * img * 8 - 1), dict(mode=EDGE, d=DUMMY + 0x100000 + 2 * img - 8)]
    for b in bad:
        a = dict(good, **b)
        rc = lib.debig_png_label_boundary(a["d"], a["o"], a["n"], a["w"], a["h"], a["dtype"], a["r"], a["shape"], a["mode"], a["value"], a["status"])
        assert rc == BAD_ARG, b
    # n == 0 is fine and touches nothing, whatever else is passed
    assert lib.debig_png_label_boundary(None, None, 0, 0, 0, 9, 0, 9, 9, 0, None) == 0
    assert lib.debig_png_label_boundary(DUMMY, DUMMY, 0, 33, 24, 3, 2, 0, 0, 255, None) == 0
    # every image left out: nothing to do, and still no device; ranges that only touch are no overlap, but these are never launched
    st = (C.c_uint32 * 2)(5, 1)
    assert lib.debig_png_label_boundary(DUMMY, DUMMY + 2 * img * 8, 2, 33, 24, 3, 2, 0, 0, 255, st) == 0
    assert lib.debig_png_label_boundary(DUMMY + 2 * img, DUMMY, 2, 33, 24, 3, 2, 0, EDGE, 2 ** 40, st) == 0  # EDGE ignores the value


# ---- Python ------------------------------------------------------------------------------------------------------------------------------

def test_png_label_boundary_argument_rules(api):
    import torch

    ok = torch.zeros((2, 4, 5), dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        api.png_label_boundary(ok)
    for r in (0, 17, -1, 2.0, "1", None, True):
        with pytest.raises(ValueError, match="radius"):
            api.png_label_boundary(ok, radius=r)
    for s in ("circle", 1, None):
        with pytest.raises(ValueError, match="shape"):
            api.png_label_boundary(ok, shape=s)
    for m in ("inner", 0, None):
        with pytest.raises(ValueError, match="mode"):
            api.png_label_boundary(ok, mode=m)
    for dt, values in ((torch.uint8, (256, -1)), (torch.int16, (65536, -1)), (torch.int32, (2 ** 31, -2 ** 31 - 1)), (torch.int64, (2 ** 63, 1.0, "7", None, True))):
        for v in values:
            with pytest.raises(ValueError, match="value"):
                api.png_label_boundary(torch.zeros((2, 4, 5), dtype=dt), value=v)
        with pytest.raises(ValueError, match="GPU"):  # ... and under "edge" the value is not looked at
            api.png_label_boundary(torch.zeros((2, 4, 5), dtype=dt), mode="edge", value=values[0])
    for t in (torch.zeros((4, 5), dtype=torch.int64), torch.zeros((1, 2, 4, 5), dtype=torch.int64), np.zeros((2, 4, 5), np.int64)):
        with pytest.raises(ValueError, match=r"\(N, H, W\)"):
            api.png_label_boundary(t)
    for dt in (torch.float32, torch.int8, torch.bool, torch.float16):
        with pytest.raises(ValueError, match="uint8, uint16"):
            api.png_label_boundary(torch.zeros((2, 4, 5), dtype=dt))
    with pytest.raises(ValueError, match="contiguous"):
        api.png_label_boundary(torch.zeros((2, 5, 4), dtype=torch.int32).transpose(1, 2))
    assert api.PNG_LABEL_BOUNDARY_MAX_RADIUS == 16
    sig = inspect.signature(api.png_label_boundary)
    assert list(sig.parameters) == ["labels", "radius", "shape", "mode", "value", "status"]
    assert [p.default for p in sig.parameters.values()][1:] == [1, "square", "ring", 255, None]
    assert list(inspect.signature(api.png_label_boundary_reach).parameters) == ["radius", "shape"]
    assert "png_label_stats" in api.png_label_boundary.__doc__


def test_the_label_decode_calls_keep_their_signatures(api):
    """the boundary is a call of its own on the tensor that came back, not a keyword of the decode calls"""
    assert list(inspect.signature(api.png_decode_batch_labels).parameters) == [
        "datas", "size", "dtype", "boxes", "lut", "fill", "device", "warp", "border", "border_label", "perspective", "elastic", "stats"]
    assert list(inspect.signature(api.png_decode_batch_color_labels).parameters) == [
        "datas", "size", "colors", "missing", "dtype", "boxes", "fill", "device", "perspective", "elastic", "stats", "warp", "border",
        "border_label"]


def test_symbols_are_exported_and_declared(lib):
    for name in ("debig_png_label_boundary", "debig_png_label_boundary_reach", "debig_hip_png_label_boundary_batch"):
        assert hasattr(lib, name), name
    pub = open(os.path.join(ROOT, "include", "decode_png.h")).read()
    dev = open(os.path.join(ROOT, "include", "debig_hip.h")).read()
    for text in ("int debig_png_label_boundary(", "void debig_png_label_boundary_reach(uint32_t radius, uint32_t shape, uint8_t reach[17]);",
                 "DEBIG_PNG_BOUNDARY_SQUARE 0u", "DEBIG_PNG_BOUNDARY_DIAMOND 1u", "DEBIG_PNG_BOUNDARY_DISK 2u", "DEBIG_PNG_BOUNDARY_RING 0u",
                 "DEBIG_PNG_BOUNDARY_EDGE 1u"):
        assert text in pub, text
    for text in ("int debig_hip_png_label_boundary_batch(", "} debig_png_label_boundary_task;", "DEBIG_PNG_LABEL_BOUNDARY_MAX_RADIUS 16u",
                 "_blur, _label_stats and"):
        assert text in dev, text


# ---- the sanitizer program (stand-alone, a plain child process) --------------------------------------------------------------------------

def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    r = subprocess.run(["sh", os.path.join(ROOT, "tools", "asan_png_label_boundary_emu.sh"), str(tmp_path)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
