"""The label distance without a GPU (include/decode_png.h: debig_png_label_distance): the brute-force numpy restatement
tests/png_label_distance_ref.py on maps worked out by hand, against scipy's distance_transform_edt (TO_VALUE) and against the boundary
restatement with the disk (DIFFERS), the separable form of DESIGN.md against the brute force, every argument check of the C call that
is decided before a device is touched, the argument rules of png_label_distance, the unchanged signatures of the label decode calls
and of png_label_boundary, the new symbols, and the stand-alone sanitizer program of the two kernels on the emulator."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_boundary_ref as B  # noqa: E402
import png_label_distance_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -2
DUMMY = 0x10000  # "device pointers" that are never followed: every case below is refused before a device is touched
DIFFERS, TO_VALUE, SQUARED, ROOT_F = 0, 1, 0, 1


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
    L.debig_png_label_distance.restype = C.c_int
    L.debig_png_label_distance.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_int64, C.c_uint32, C.c_uint32, C.c_void_p]
    return L


def _maps():
    rng = np.random.default_rng(0)
    out = []
    for H, W in ((1, 1), (1, 7), (9, 1), (3, 4), (16, 24), (11, 13)):
        out.append(rng.integers(0, 3, (H, W)).astype(np.int32))  # random
        out.append(np.repeat(np.repeat(rng.integers(0, 4, (-(-H // 4), -(-W // 5))), 4, axis=0), 5, axis=1)[:H, :W].astype(np.int32))  # blocky
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def test_the_restatement_on_maps_worked_out_by_hand():
    img = np.array([[1, 1, 1, 1, 1],
                    [1, 1, 1, 1, 1],
                    [1, 1, 2, 1, 1],
                    [1, 1, 1, 1, 1]], np.int32)
    d, none = R.d2(img, 2)
    assert not none.any() and d.tolist() == [[8, 5, 4, 5, 8],
                                             [5, 2, 1, 2, 5],
                                             [4, 1, 0, 1, 4],
                                             [5, 2, 1, 2, 5]]
    dd, none = R.d2(img)
    want = d.copy()
    want[2, 2] = 1  # the lone element's nearest differing element is a neighbour
    assert not none.any() and np.array_equal(dd, want)
    assert R.apply_image(img, 2, 2).tolist() == [[4, 4, 4, 4, 4], [4, 2, 1, 2, 4], [4, 1, 0, 1, 4], [4, 2, 1, 2, 4]]
    root = R.apply_image(img, 2, None, "root")
    assert root.dtype == np.float32 and root[0, 0] == np.float32(np.sqrt(8.0)) and root[2, 2] == 0 and root[0, 2] == 2
    # two classes: both halves of a signed distance at once
    two = np.array([[0, 0, 0, 7, 7, 7]], np.uint8)
    assert R.apply_image(two).tolist() == [[9, 4, 1, 1, 4, 9]] and R.apply_image(two, 7).tolist() == [[9, 4, 1, 0, 0, 0]]
    # NONE: a flat image under DIFFERS, an absent value under TO_VALUE; with and without a cap, both formats
    flat = np.full((3, 4), 5, np.int64)
    for to in (None, 6):
        assert R.d2(flat, to)[1].all()
        assert (R.apply_image(flat, to) == 2 ** 31 - 1).all() and R.apply_image(flat, to).dtype == np.int32
        assert np.isposinf(R.apply_image(flat, to, None, "root")).all()
        assert (R.apply_image(flat, to, 5) == 25).all() and (R.apply_image(flat, to, 5, "root") == 5.0).all()
    assert (R.apply_image(flat, 5) == 0).all() and (R.apply_image(np.array([[4]])) == 2 ** 31 - 1).all()
    # elements are compared whole; a value the dtype cannot hold matches nothing
    big = np.array([[3, 2 ** 32 + 3, 3]], np.int64)
    assert R.apply_image(big).tolist() == [[1, 1, 1]] and R.apply_image(big, 3).tolist() == [[0, 1, 0]]
    assert R.apply_image(np.array([[-1, 255]], np.int32)).tolist() == [[1, 1]]
    assert R.d2(np.array([[255, 1]], np.uint8), -1)[1].all() and R.d2(np.array([[255, 1]], np.uint8), 256)[1].all()
    assert R.apply_image(np.array([[-1, 7]], np.int16), 65535).tolist() == [[0, 1]]  # int16 is the uint16 bits
    # a skipped image comes back as zeros
    both = np.stack([img, img])
    res = R.apply(both, 2, None, "squared", status=[3, 0])
    assert not res[0].any() and np.array_equal(res[1], d)
    # the g plane of the rows kernel
    g = R.row_g(np.array([[1, 1, 2, 2, 2], [1, 1, 1, 1, 1], [1, 2, 1, 1, 1]], np.uint8))
    N, A = R.G_NONE, R.G_ABOVE
    assert g.tolist() == [[2, 1, 1, 2, 3], [N, N, N | A, N | A, N | A], [1, 1 | A, 1, 2, 3]]
    assert R.row_g(np.array([[1, 1, 2, 2, 2], [1, 1, 1, 1, 1]], np.uint8), 2).tolist() == [[2, 1, 0, 0, 0], [N] * 5]


def test_the_root_is_the_nearest_float32_and_sqrtf_of_a_float_is_not():
    """(float)sqrt((double)d2) against exact integer arithmetic: the float32 f is the nearest to sqrt(d2) iff d2 lies between the
    squares of the two midpoints around f, which are exact in float64 (25 bits, squared 50)"""
    k = np.arange(4097, 16384, 7, dtype=np.int64)
    d2 = np.concatenate([k * k + 1, k * k + 4, k * k - 1, k * k + k])
    f = R.finish(d2, np.zeros(d2.shape, bool), None, "root")
    lo = (f.astype(np.float64) + np.nextafter(f, np.float32(0)).astype(np.float64)) / 2
    hi = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    assert ((lo * lo < d2) & (d2 < hi * hi)).all()
    assert (np.sqrt(d2.astype(np.float32)) != f).any()  # rounding the argument first is another rule


def test_to_value_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for img in _maps():
        for v in (0, 1, 3):
            d, none = R.d2(img, v)
            if not (img == v).any():
                assert none.all()
                continue
            edt = ndi.distance_transform_edt(img != v)
            assert not none.any() and np.array_equal(d, np.rint(edt * edt).astype(np.int64)), (img.shape, v)
            assert np.array_equal(R.apply_image(img, v, None, "root"), np.sqrt(d.astype(np.float64)).astype(np.float32))


def test_differs_against_the_boundary_restatement_with_the_disk():
    """D2 <= r^2 is the EDGE map of the disk of radius r, for every radius the boundary call has"""
    for img in _maps():
        d, none = R.d2(img)
        for r in range(1, B.MAX_RADIUS + 1):
            assert np.array_equal((d <= r * r) & ~none, B.boundary(img, B.reach(r, "disk"))), (img.shape, r)
        assert np.array_equal(R.apply_image(img, None, 16) < 256, (d < 256) & ~none)


def test_the_separable_form_against_the_brute_force():
    for img in _maps() + [np.array([[1], [1], [2], [1], [1], [1]]), np.array([[0, 1], [1, 0], [0, 1]])]:
        for to in (None, 0, 1, 9):
            d, none = R.d2(img, to)
            ds, ns = R.separable(img, to)
            assert np.array_equal(none, ns) and np.array_equal(d[~none], ds[~ns]), (img.shape, to)


# ---- the C call's argument checks --------------------------------------------------------------------------------------------------------

def test_c_argument_checks_come_before_any_device_work(lib):
    img = 33 * 24
    good = dict(d=DUMMY, o=DUMMY + 0x100000, n=2, w=33, h=24, dtype=3, sites=DIFFERS, value=0, cap=0, fmt=SQUARED, status=None)
    bad = [dict(d=None), dict(o=None), dict(d=DUMMY + 4), dict(o=DUMMY + 0x100002), dict(o=DUMMY + 0x100001), dict(d=DUMMY + 1, dtype=1),
           dict(d=DUMMY + 2, dtype=2), dict(dtype=4), dict(dtype=2 ** 31), dict(sites=2), dict(sites=2 ** 31), dict(fmt=2), dict(fmt=2 ** 31),
           dict(cap=32768), dict(cap=2 ** 32 - 1), dict(w=0), dict(w=16385), dict(h=0), dict(h=16385),
           dict(o=DUMMY), dict(o=DUMMY + 8), dict(o=DUMMY + 2 * img * 8 - 8), dict(d=DUMMY + 0x100000 + 2 * img * 4 - 8),
           dict(dtype=0, o=DUMMY + 2 * img - 4), dict(dtype=0, d=DUMMY + 0x100000 + 2 * img * 4 - 1)]
    for b in bad:
        a = dict(good, **b)
        rc = lib.debig_png_label_distance(a["d"], a["o"], a["n"], a["w"], a["h"], a["dtype"], a["sites"], a["value"], a["cap"], a["fmt"],
                                          a["status"])
        assert rc == BAD_ARG, b
    # n == 0 is fine and touches nothing, whatever else is passed
    assert lib.debig_png_label_distance(None, None, 0, 0, 0, 9, 9, 0, 2 ** 31, 9, None) == 0
    assert lib.debig_png_label_distance(DUMMY, DUMMY, 0, 33, 24, 3, 0, 0, 0, 0, None) == 0
    # every image left out: nothing to do, and still no device; ranges that only touch are no overlap.  A value that the dtype
    # cannot hold is not an error, and neither is the largest cap
    st = (C.c_uint32 * 2)(5, 1)
    assert lib.debig_png_label_distance(DUMMY, DUMMY + 2 * img * 8, 2, 33, 24, 3, 0, 0, 0, 0, st) == 0
    assert lib.debig_png_label_distance(DUMMY + 2 * img * 4, DUMMY, 2, 33, 24, 0, TO_VALUE, 2 ** 40, 32767, ROOT_F, st) == 0
    assert lib.debig_png_label_distance(DUMMY + 2 * img * 4, DUMMY, 2, 33, 24, 1, TO_VALUE, -1, 1, SQUARED, st) == 0


# ---- Python ------------------------------------------------------------------------------------------------------------------------------

def test_png_label_distance_argument_rules(api):
    import torch

    ok = torch.zeros((2, 4, 5), dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        api.png_label_distance(ok)
    for to in (1.0, "1", True, 2 ** 63, -2 ** 63 - 1, (1,)):
        with pytest.raises(ValueError, match="to must"):
            api.png_label_distance(ok, to=to)
    for cap in (0, 32768, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="cap"):
            api.png_label_distance(ok, cap=cap)
    for out in ("sqrt", 0, None, "SQUARED"):
        with pytest.raises(ValueError, match="out"):
            api.png_label_distance(ok, out=out)
    for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):  # a value the dtype cannot hold is no error: the next check is reached
        with pytest.raises(ValueError, match="GPU"):
            api.png_label_distance(torch.zeros((2, 4, 5), dtype=dt), to=2 ** 40, cap=32767, out="root")
        with pytest.raises(ValueError, match="GPU"):
            api.png_label_distance(torch.zeros((2, 4, 5), dtype=dt), to=-1, cap=1)
    for t in (torch.zeros((4, 5), dtype=torch.int64), torch.zeros((1, 2, 4, 5), dtype=torch.int64), np.zeros((2, 4, 5), np.int64)):
        with pytest.raises(ValueError, match=r"\(N, H, W\)"):
            api.png_label_distance(t)
    for dt in (torch.float32, torch.int8, torch.bool, torch.float16):
        with pytest.raises(ValueError, match="uint8, uint16"):
            api.png_label_distance(torch.zeros((2, 4, 5), dtype=dt))
    with pytest.raises(ValueError, match="contiguous"):
        api.png_label_distance(torch.zeros((2, 5, 4), dtype=torch.int32).transpose(1, 2))
    assert api.PNG_LABEL_DISTANCE_MAX_CAP == 32767
    sig = inspect.signature(api.png_label_distance)
    assert list(sig.parameters) == ["labels", "to", "cap", "out", "status"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, None, "squared", None]
    assert "png_label_boundary" in api.png_label_distance.__doc__ and "distance_transform_edt" in api.png_label_distance.__doc__


def test_the_existing_calls_keep_their_signatures(api):
    """the distance is a call of its own on the tensor that came back, not a keyword of the decode calls"""
    assert list(inspect.signature(api.png_decode_batch_labels).parameters) == [
        "datas", "size", "dtype", "boxes", "lut", "fill", "device", "warp", "border", "border_label", "perspective", "elastic", "stats"]
    assert list(inspect.signature(api.png_decode_batch_color_labels).parameters) == [
        "datas", "size", "colors", "missing", "dtype", "boxes", "fill", "device", "perspective", "elastic", "stats", "warp", "border",
        "border_label"]
    assert list(inspect.signature(api.png_label_boundary).parameters) == ["labels", "radius", "shape", "mode", "value", "status"]
    assert list(inspect.signature(api.png_label_stats).parameters) == ["labels", "num_ids", "status"]


def test_symbols_are_exported_and_declared(lib):
    for name in ("debig_png_label_distance", "debig_hip_png_label_distance_rows_batch", "debig_hip_png_label_distance_cols_batch"):
        assert hasattr(lib, name), name
    pub = open(os.path.join(ROOT, "include", "decode_png.h")).read()
    dev = open(os.path.join(ROOT, "include", "debig_hip.h")).read()
    for text in ("int debig_png_label_distance(", "DEBIG_PNG_DISTANCE_DIFFERS 0u", "DEBIG_PNG_DISTANCE_TO_VALUE 1u", "DEBIG_PNG_DISTANCE_SQUARED 0u",
                 "DEBIG_PNG_DISTANCE_ROOT 1u", "(float)sqrt((double)d2)"):
        assert text in pub, text
    for text in ("int debig_hip_png_label_distance_rows_batch(", "int debig_hip_png_label_distance_cols_batch(",
                 "} debig_png_label_distance_rows_task;", "} debig_png_label_distance_cols_task;", "_label_distance_rows / _label_distance_cols --"):
        assert text in dev, text


# ---- the sanitizer program (stand-alone, a plain child process) --------------------------------------------------------------------------

def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    r = subprocess.run(["sh", os.path.join(ROOT, "tools", "asan_png_label_distance_emu.sh"), str(tmp_path)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
