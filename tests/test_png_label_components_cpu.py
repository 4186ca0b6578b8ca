"""The label components without a GPU (include/decode_png.h: debig_png_label_components): the numpy restatement
tests/png_label_components_ref.py (a fixpoint of minima) on maps worked out by hand and against scipy.ndimage.label value by value with
the matching structure -- the partition AND the numbering --, every argument check of the C call that is decided before a device is
touched, the argument rules of png_label_components, the unchanged signatures of its siblings, the new symbols, and the stand-alone
sanitizer program of the five kernels on the emulator."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_components_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -2
DUMMY = 0x10000  # "device pointers" that are never followed: every case below is refused before a device is touched
FIRST, CONSECUTIVE = 0, 1


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
    L.debig_png_label_components.restype = C.c_int
    L.debig_png_label_components.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def test_the_restatement_on_maps_worked_out_by_hand():
    img = np.array([[1, 1, 0, 2],
                    [0, 1, 0, 2],
                    [1, 0, 2, 0],
                    [1, 0, 0, 0]], np.int32)
    f4 = R.first(img, 4)
    assert f4.tolist() == [[0, 0, 2, 3], [4, 0, 2, 3], [8, 9, 10, 9], [8, 9, 9, 9]]  # the zeros of the last rows meet in the corner
    c4, k4 = R.consecutive(f4)
    assert k4 == 7 and c4.tolist() == [[1, 1, 2, 3], [4, 1, 2, 3], [5, 6, 7, 6], [5, 6, 6, 6]]
    f8 = R.first(img, 8)
    assert f8.tolist() == [[0, 0, 2, 3], [2, 0, 2, 3], [0, 2, 3, 2], [0, 2, 2, 2]]  # every value is one component through corners
    assert R.consecutive(f8)[1] == 3
    # a background belongs to no component: -1 / 0
    b4 = R.first(img, 4, 0)
    assert b4.tolist() == [[0, 0, -1, 3], [-1, 0, -1, 3], [8, -1, 10, -1], [8, -1, -1, -1]]
    assert R.consecutive(b4)[0].tolist() == [[1, 1, 0, 2], [0, 1, 0, 2], [3, 0, 4, 0], [3, 0, 0, 0]] and R.consecutive(b4)[1] == 4
    b8 = R.first(img, 8, 0)
    assert R.consecutive(b8)[0].tolist() == [[1, 1, 0, 2], [0, 1, 0, 2], [1, 0, 2, 0], [1, 0, 0, 0]]
    # elements are compared whole; a background that the dtype cannot hold matches nothing; int16 is the uint16 bits
    big = np.array([[3, 2 ** 32 + 3, 3]], np.int64)
    assert R.first(big, 8).tolist() == [[0, 1, 2]] and R.first(big, 8, 3).tolist() == [[-1, 1, -1]]
    assert R.first(np.array([[-1, 255, 255]], np.int32), 4, 255).tolist() == [[0, -1, -1]]
    assert R.first(np.array([[255, 255, 1]], np.uint8), 4, -1).tolist() == [[0, 0, 2]]
    assert R.first(np.array([[255, 255, 1]], np.uint8), 4, 256 + 255).tolist() == [[0, 0, 2]]
    assert R.first(np.array([[-1, -1, 7]], np.int16), 4, 65535).tolist() == [[-1, -1, 2]]
    # a skipped image comes back as zeros with a count of 0
    out, counts = R.apply(np.stack([img, img]), 4, 0, "consecutive", status=[3, 0])
    assert not out[0].any() and counts.tolist() == [0, 4] and out[1].tolist() == R.consecutive(b4)[0].tolist()
    out, counts = R.apply(np.stack([img, img]), 8, None, "first")
    assert out[0].tolist() == f8.tolist() and counts.tolist() == [3, 3] and out.dtype == np.int32 and counts.dtype == np.int64


def _maps(dtype):
    rng = np.random.default_rng(0)
    out = []
    for H, W in ((1, 1), (1, 7), (9, 1), (3, 4), (16, 24), (11, 13), (40, 70)):
        out.append(rng.integers(0, 3, (H, W)).astype(dtype))  # random
        out.append(np.repeat(np.repeat(rng.integers(0, 4, (-(-H // 4), -(-W // 5))), 4, axis=0), 5, axis=1)[:H, :W].astype(dtype))  # blocky
    return out


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16, np.int32, np.int64])
def test_the_partition_and_the_numbering_against_scipy(dtype):
    """value by value with the matching structure: the restatement's FIRST is constant on every scipy component, differs between
    them, and is the component's first element in raster order; on a binary mask with background 0 the consecutive numbers ARE
    scipy's labels"""
    ndi = pytest.importorskip("scipy.ndimage")
    structures = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: np.ones((3, 3), int)}
    for img in _maps(dtype):
        for connectivity, st in structures.items():
            fst = R.first(img, connectivity)
            total = 0
            for v in np.unique(img):
                lab, k = ndi.label(img == v, structure=st)
                total += k
                for c in range(1, k + 1):
                    m = lab == c
                    assert (fst[m] == np.flatnonzero(m.ravel())[0]).all(), (img.shape, connectivity, v, c)
                # the value alone, everything else background: the numbering is scipy's
                mask = (img == v).astype(dtype)
                cons, kk = R.consecutive(R.first(mask, connectivity, 0))
                assert kk == k and np.array_equal(cons, lab), (img.shape, connectivity, v)
            assert R.consecutive(fst)[1] == total
            # ... and with that value as the background of the whole map
            v = int(np.unique(img)[0])
            bf = R.first(img, connectivity, v)
            assert np.array_equal(bf, np.where(img == v, -1, fst))


# ---- the C call's argument checks --------------------------------------------------------------------------------------------------------

def test_c_argument_checks_come_before_any_device_work(lib):
    img = 33 * 24
    good = dict(d=DUMMY, o=DUMMY + 0x100000, n=2, w=33, h=24, dtype=3, conn=4, use=0, bg=0, ids=CONSECUTIVE, status=None, counts=None)
    bad = [dict(d=None), dict(o=None), dict(d=DUMMY + 4), dict(o=DUMMY + 0x100002), dict(o=DUMMY + 0x100001), dict(d=DUMMY + 1, dtype=1),
           dict(d=DUMMY + 2, dtype=2), dict(dtype=4), dict(dtype=2 ** 31), dict(conn=0), dict(conn=1), dict(conn=2), dict(conn=6), dict(conn=12),
           dict(conn=2 ** 32 - 4), dict(ids=2), dict(ids=2 ** 31), dict(w=0), dict(w=16385), dict(h=0), dict(h=16385),
           dict(o=DUMMY), dict(o=DUMMY + 8), dict(o=DUMMY + 2 * img * 8 - 8), dict(d=DUMMY + 0x100000 + 2 * img * 4 - 8),
           dict(dtype=0, o=DUMMY + 2 * img - 4), dict(dtype=0, d=DUMMY + 0x100000 + 2 * img * 4 - 1)]
    for b in bad:
        a = dict(good, **b)
        counts = (C.c_uint32 * 2)(7, 7)
        rc = lib.debig_png_label_components(a["d"], a["o"], a["n"], a["w"], a["h"], a["dtype"], a["conn"], a["use"], a["bg"], a["ids"],
                                            a["status"], counts)
        assert rc == BAD_ARG and list(counts) == [7, 7], b
    # n == 0 is fine and touches nothing, whatever else is passed
    assert lib.debig_png_label_components(None, None, 0, 0, 0, 9, 9, 9, 0, 9, None, None) == 0
    assert lib.debig_png_label_components(DUMMY, DUMMY, 0, 33, 24, 3, 4, 0, 0, 0, None, None) == 0
    # every image left out: nothing to do, counts of 0, and still no device; ranges that only touch are no overlap.  A background
    # that the dtype cannot hold is not an error
    st = (C.c_uint32 * 2)(5, 1)
    counts = (C.c_uint32 * 2)(7, 7)
    assert lib.debig_png_label_components(DUMMY, DUMMY + 2 * img * 8, 2, 33, 24, 3, 8, 0, 0, FIRST, st, counts) == 0 and list(counts) == [0, 0]
    assert lib.debig_png_label_components(DUMMY + 2 * img * 4, DUMMY, 2, 33, 24, 0, 4, 1, 2 ** 40, CONSECUTIVE, st, None) == 0
    assert lib.debig_png_label_components(DUMMY + 2 * img * 4, DUMMY, 2, 33, 24, 1, 8, 1, -1, FIRST, st, None) == 0


# ---- Python ------------------------------------------------------------------------------------------------------------------------------

def test_png_label_components_argument_rules(api):
    import torch

    ok = torch.zeros((2, 4, 5), dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        api.png_label_components(ok)
    for connectivity in (0, 1, 2, 6, "4", 4.5, None, True):
        with pytest.raises(ValueError, match="connectivity"):
            api.png_label_components(ok, connectivity)
    for background in (1.0, "1", True, 2 ** 63, -2 ** 63 - 1, (1,)):
        with pytest.raises(ValueError, match="background must"):
            api.png_label_components(ok, background=background)
    for ids in ("root", 0, None, "FIRST"):
        with pytest.raises(ValueError, match="ids"):
            api.png_label_components(ok, ids=ids)
    for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):  # a value the dtype cannot hold is no error: the next check is reached
        with pytest.raises(ValueError, match="GPU"):
            api.png_label_components(torch.zeros((2, 4, 5), dtype=dt), 8, background=2 ** 40, ids="first")
        with pytest.raises(ValueError, match="GPU"):
            api.png_label_components(torch.zeros((2, 4, 5), dtype=dt), background=-1)
    for t in (torch.zeros((4, 5), dtype=torch.int64), torch.zeros((1, 2, 4, 5), dtype=torch.int64), np.zeros((2, 4, 5), np.int64)):
        with pytest.raises(ValueError, match=r"\(N, H, W\)"):
            api.png_label_components(t)
    for dt in (torch.float32, torch.int8, torch.bool, torch.float16):
        with pytest.raises(ValueError, match="uint8, uint16"):
            api.png_label_components(torch.zeros((2, 4, 5), dtype=dt))
    with pytest.raises(ValueError, match="contiguous"):
        api.png_label_components(torch.zeros((2, 5, 4), dtype=torch.int32).transpose(1, 2))
    sig = inspect.signature(api.png_label_components)
    assert list(sig.parameters) == ["labels", "connectivity", "background", "ids", "status"]
    assert [p.default for p in sig.parameters.values()][1:] == [4, None, "consecutive", None]
    doc = api.png_label_components.__doc__
    assert "png_label_stats(ids, K + 1)" in doc and "scipy.ndimage.label" in doc


def test_the_existing_calls_keep_their_signatures(api):
    """the components are a call of their own on the tensor that came back, not a keyword of the decode calls or of the stats"""
    assert list(inspect.signature(api.png_label_stats).parameters) == ["labels", "num_ids", "status"]
    assert list(inspect.signature(api.png_label_boundary).parameters) == ["labels", "radius", "shape", "mode", "value", "status"]
    assert list(inspect.signature(api.png_label_distance).parameters) == ["labels", "to", "cap", "out", "status"]


def test_symbols_are_exported_and_declared(lib):
    names = ["debig_hip_png_label_components_%s_batch" % s for s in ("rows", "merge", "count", "number", "finish")]
    for name in ["debig_png_label_components"] + names:
        assert hasattr(lib, name), name
    pub = open(os.path.join(ROOT, "include", "decode_png.h")).read()
    dev = open(os.path.join(ROOT, "include", "debig_hip.h")).read()
    for text in ("int debig_png_label_components(", "DEBIG_PNG_COMPONENTS_FIRST 0u", "DEBIG_PNG_COMPONENTS_CONSECUTIVE 1u", "fuzzy", "minimum-area",
                 "3-D labelling"):
        assert text in pub, text
    for text in ["int %s(" % n for n in names] + ["} debig_png_label_components_task;",
                                                  "_label_components_rows / _merge / _count / _number / _finish --"]:
        assert text in dev, text


# ---- the sanitizer program (stand-alone, a plain child process) --------------------------------------------------------------------------

def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    r = subprocess.run(["sh", os.path.join(ROOT, "tools", "asan_png_label_components_emu.sh"), str(tmp_path)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
