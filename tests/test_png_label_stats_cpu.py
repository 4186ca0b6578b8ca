"""The label statistics without a GPU (include/decode_png.h: debig_png_label_stats): the host's raw -> public conversion against
the numpy restatement tests/png_label_stats_ref.py, the restatement's own properties, every argument check of the C call that is
decided before a device is touched, the argument rules of png_label_stats and of the decode calls' stats= keyword, the new symbols,
and the stand-alone sanitizer program of the kernel on the emulator."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_stats_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -2
DUMMY = 0x1000  # a "device pointer" that is never followed: every case below is refused before a device is touched


class Box(C.Structure):  # include/decode_png.h: debig_png_label_box
    _fields_ = [("count", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32)]


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
    L.debig_png_label_stat_box.restype = None
    L.debig_png_label_stat_box.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(Box)]
    L.debig_png_label_stats.restype = C.c_int
    L.debig_png_label_stats.argtypes = [C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p, C.c_void_p]
    return L


def _host_box(lib, raw, W, H):
    b = Box(9, 9, 9, 9, 9)
    lib.debig_png_label_stat_box((C.c_uint32 * 5)(*[int(v) for v in raw]), W, H, C.byref(b))
    return [b.count, b.x0, b.y0, b.x1, b.y1]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def test_the_restatement_on_a_map_worked_out_by_hand(lib):
    img = np.array([[0, 0, 2, 2],
                    [0, 7, 2, -1],
                    [5, 5, 5, 255]], np.int32)
    s = R.stats(img[None], 4)[0]
    assert s.tolist() == [[3, 0, 0, 2, 2], [0] * 5, [3, 2, 0, 4, 2], [0] * 5, [6, 0, 1, 4, 3]]  # 7, -1, 5 x 3 and 255 are "other"
    raw = R.to_raw(s, 4, 3)  # ... and as the device keeps them: count, max x + 1, max y + 1, out_w - min x, out_h - min y
    assert raw.tolist() == [[3, 2, 2, 4, 3], [0] * 5, [3, 4, 2, 2, 3], [0] * 5, [6, 4, 3, 4, 2]]
    assert [_host_box(lib, r, 4, 3) for r in raw] == s.tolist()
    assert R.stats(img[None], 8)[0][7].tolist() == [1, 1, 1, 2, 2] and R.stats(img[None], 8)[0][8].tolist() == [2, 3, 1, 4, 3]
    assert not R.stats(img[None], 4, status=[3]).any()
    big = np.array([[2 ** 32 + 3, 3, -2 ** 63, 2 ** 40]], np.int64)
    assert R.stats(big[None], 4)[0].tolist() == [[0] * 5] * 3 + [[1, 1, 0, 2, 1], [3, 0, 0, 4, 1]]
    as16 = np.array([[65535, 3]], np.uint16).view(np.int16)  # uint16 handed out as int16 bits: -1 reads as 65535
    assert R.stats(as16[None], 4)[0][4].tolist() == [1, 0, 0, 1, 1]
    # counts of all records sum to the image; every box holds its count
    rng = np.random.default_rng(0)
    lab = rng.integers(-2, 30, (3, 24, 33)).astype(np.int64)
    s = R.stats(lab, 21)
    assert (s[..., 0].sum(axis=1) == 24 * 33).all()
    assert ((s[..., 3] - s[..., 1]) * (s[..., 4] - s[..., 2]) >= s[..., 0]).all()


# ---- the host's conversion ----------------------------------------------------------------------------------------------------------------

def test_host_conversion_against_the_restatement(lib):
    for W, H in ((1, 1), (33, 24), (16384, 16384), (70, 1)):
        corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]  # 1-pixel boxes at all four corners
        boxes = [[1, x, y, x + 1, y + 1] for x, y in corners] + [[W * H, 0, 0, W, H], [0, 0, 0, 0, 0]]
        if W > 2 and H > 2:
            boxes += [[5, 1, 2, W - 1, H], [2, 0, 1, 2, 2]]
        pub = np.array(boxes, np.int64)
        raw = R.to_raw(pub, W, H)
        assert raw.dtype == np.uint32 and np.array_equal(R.to_public(raw, W, H), pub)
        for r, p in zip(raw, pub):
            assert _host_box(lib, r, W, H) == p.tolist(), (W, H, p)
        assert raw[0].tolist() == [1, 1, 1, W, H] and raw[3].tolist() == [1, W, H, 1, 1] and not raw[5].any()
    # an empty record is empty whatever its extremes hold
    assert _host_box(lib, [0, 7, 7, 7, 7], 33, 24) == [0, 0, 0, 0, 0]
    # random maps: restatement -> raw -> host == restatement
    rng = np.random.default_rng(1)
    lab = rng.integers(0, 12, (2, 9, 13)).astype(np.uint8)
    pub = R.stats(lab, 8)
    raw = R.to_raw(pub, 13, 9)
    for i in range(2):
        for k in range(9):
            assert _host_box(lib, raw[i, k], 13, 9) == pub[i, k].tolist()


def test_c_argument_checks_leave_out_unwritten(lib):
    out = (Box * 44)()
    C.memset(out, 0xEE, C.sizeof(out))
    before = bytes(out)
    good = dict(d=DUMMY, n=2, w=33, h=24, dtype=3, ids=21, status=None, out=out)
    bad = [dict(ids=0), dict(ids=1025), dict(ids=2 ** 32 - 1), dict(dtype=4), dict(dtype=2 ** 31), dict(w=0), dict(w=16385), dict(h=0),
           dict(h=16385), dict(out=None), dict(d=None), dict(d=DUMMY + 4), dict(d=DUMMY + 1, dtype=1), dict(d=DUMMY + 2, dtype=2)]
    for b in bad:
        a = dict(good, **b)
        assert lib.debig_png_label_stats(a["d"], a["n"], a["w"], a["h"], a["dtype"], a["ids"], a["status"], a["out"]) == BAD_ARG, b
        assert bytes(out) == before
    # n == 0 is fine and touches nothing, whatever else is passed
    assert lib.debig_png_label_stats(None, 0, 0, 0, 9, 0, None, None) == 0
    assert lib.debig_png_label_stats(DUMMY, 0, 33, 24, 3, 21, None, out) == 0 and bytes(out) == before
    # every image left out: zero records, and still no device
    st = (C.c_uint32 * 2)(5, 1)
    assert lib.debig_png_label_stats(DUMMY, 2, 33, 24, 3, 21, st, out) == 0 and not any(bytes(out))


# ---- Python ------------------------------------------------------------------------------------------------------------------------------

def test_png_label_stats_argument_rules(api):
    import torch

    ok = torch.zeros((2, 4, 5), dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        api.png_label_stats(ok, 21)
    for ids in (0, 1025, -1, 2.0, "21", None, True):
        with pytest.raises(ValueError, match="num_ids"):
            api.png_label_stats(ok, ids)
    for t in (torch.zeros((4, 5), dtype=torch.int64), torch.zeros((1, 2, 4, 5), dtype=torch.int64), np.zeros((2, 4, 5), np.int64)):
        with pytest.raises(ValueError, match=r"\(N, H, W\)"):
            api.png_label_stats(t, 21)
    for dt in (torch.float32, torch.int8, torch.bool, torch.float16):
        with pytest.raises(ValueError, match="uint8, uint16"):
            api.png_label_stats(torch.zeros((2, 4, 5), dtype=dt), 21)
    with pytest.raises(ValueError, match="contiguous"):
        api.png_label_stats(torch.zeros((2, 5, 4), dtype=torch.int32).transpose(1, 2), 21)
    with pytest.raises(ValueError, match="contiguous"):
        api.png_label_stats(torch.zeros((2, 4, 10), dtype=torch.uint8)[:, :, ::2], 21)
    assert api.PNG_LABEL_STATS_MAX_IDS == 1024
    assert list(inspect.signature(api.png_label_stats).parameters) == ["labels", "num_ids", "status"]


def test_stats_is_the_last_new_keyword_of_both_label_calls(api):
    """by name, default None, and no older parameter moves: the last parameter of png_decode_batch_labels; in
    png_decode_batch_color_labels the last of the keywords added since `warp`, in front of `warp`, `border` and `border_label`,
    which tests/test_png_color_labels_warp_cpu.py keeps as that call's last three"""
    for fn in (api.png_decode_batch_labels, api.png_decode_batch_color_labels):
        params = inspect.signature(fn).parameters
        assert params["stats"].default is None
        for bad in (0, 1025, -3, 21.0, "21", True):
            with pytest.raises(ValueError, match="num_ids"):
                fn([b""], (4, 4), stats=bad)
    assert list(inspect.signature(api.png_decode_batch_labels).parameters) == [
        "datas", "size", "dtype", "boxes", "lut", "fill", "device", "warp", "border", "border_label", "perspective", "elastic", "stats"]
    assert list(inspect.signature(api.png_decode_batch_color_labels).parameters) == [
        "datas", "size", "colors", "missing", "dtype", "boxes", "fill", "device", "perspective", "elastic", "stats", "warp", "border",
        "border_label"]


def test_symbols_are_exported_and_declared(lib):
    for name in ("debig_png_label_stats", "debig_png_label_stat_box", "debig_hip_png_label_stats_batch"):
        assert hasattr(lib, name), name
    pub = open(os.path.join(ROOT, "include", "decode_png.h")).read()
    dev = open(os.path.join(ROOT, "include", "debig_hip.h")).read()
    for text in ("int debig_png_label_stats(", "void debig_png_label_stat_box(", "typedef struct debig_png_label_box { uint32_t count, x0, y0, x1, y1; }"):
        assert text in pub, text
    for text in ("int debig_hip_png_label_stats_batch(", "} debig_png_label_stat;", "} debig_png_label_stats_task;", "DEBIG_PNG_LABEL_STATS_MAX_IDS 1024u"):
        assert text in dev, text


# ---- the sanitizer program (stand-alone, a plain child process) --------------------------------------------------------------------------

def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    r = subprocess.run(["sh", os.path.join(ROOT, "tools", "asan_png_label_stats_emu.sh"), str(tmp_path)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
