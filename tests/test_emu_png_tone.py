"""The two kernels of the tone curves (csrc/png_tone_kernel.inc) on the CPU lock-step emulator, BIT FOR BIT against the numpy
restatement tests/png_tone_ref.py:
  * 8-bit HWC intermediates of 67 x 19 (an odd width for the CHW byte stores) and 70 x 67, with 1, 2, 3 and 4 channels, cut into
    runs of 256 pixels: an image spans 5 or more tasks; runs of 255 pixels, so that an RGB run starts at every byte alignment;
  * one launch holds several files with different ops and deliberately different histograms (noise, a flat image, an image of
    0 and 255 only, a narrow band), so that reading another file's histogram or table shows;
  * the histogram buffer is compared on its own; every dtype, both layouts; a sentinel around the tensor and in the slots of
    skipped tasks stays; tasks that break a bound are skipped; fewer workgroups than tasks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_resize_ref as Z  # noqa: E402
import png_tone_ref as T  # noqa: E402
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402

FILL, GAP = 0xEE, 4096
SCALE, BIAS = (1 / 0.229, 1 / 0.224, 1 / 0.225, 3.0), (-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225, 0.25)
DTYPES = ["uint", "float32", "float16", "bfloat16"]
SIZES = [(19, 67), (67, 70)]  # (H, W)
RUN = 256


class ToneTask(C.Structure):  # include/debig_hip.h: debig_png_tone_task
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("hist_off", C.c_uint64), ("lut_off", C.c_uint64),
                ("pix0", C.c_uint32), ("pix_n", C.c_uint32), ("out_w", C.c_uint32), ("out_h", C.c_uint32), ("out_sx", C.c_uint32),
                ("out_sy", C.c_uint32), ("out_sc", C.c_uint32), ("channels", C.c_uint8), ("colour_channels", C.c_uint8),
                ("dtype", C.c_uint8), ("op", C.c_uint8), ("a", C.c_float * 4), ("b", C.c_float * 4)]


assert C.sizeof(ToneTask) == 96
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        L.emu_png_tone_hist_batch.restype = C.c_int
        L.emu_png_tone_hist_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.emu_png_tone_apply_batch.restype = C.c_int
        L.emu_png_tone_apply_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def _gamma():
    return np.array([min(255, int(255.0 * (i / 255.0) ** 0.5 + 0.5)) for i in range(256)], np.uint8)


def _files(size, ch):
    """[(img8, op, param, user table)]: every op, histograms that differ from file to file"""
    H, W = size
    rng = np.random.default_rng(1000 * ch + W)
    noise = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
    band = rng.integers(40, 200, (H, W, ch), dtype=np.uint8)  # lo > 0, hi < 255
    band[..., 0] = (band[..., 0] // 16) * 16
    flat = np.full((H, W, ch), 77, np.uint8)
    flat[..., -1] = 200
    two = (rng.integers(0, 2, (H, W, ch), dtype=np.uint8) * 255).astype(np.uint8)
    skew = (rng.integers(0, 256, (H, W, ch)).astype(np.float64) ** 2 / 256).astype(np.uint8)
    return [(noise, T.EQUALIZE, 0, None), (band, T.AUTOCONTRAST, 0, None), (flat, T.EQUALIZE, 0, None), (two, T.EQUALIZE, 0, None),
            (flat, T.AUTOCONTRAST, 0, None), (skew, T.POSTERIZE, 3, None), (band, T.EQUALIZE, 0, None), (noise, T.SOLARIZE, 100, None),
            (skew, T.TABLE, 0, _gamma()), (two, T.AUTOCONTRAST, 0, None), (skew, T.EQUALIZE, 0, None)]


def run(files, size, dtype, layout, run_len=RUN, grid=0, spoil=None):
    """-> (the dense tensor, the histogram buffer (n_hist_files, cc, 256), the number of tasks)"""
    H, W = size
    ch = files[0][0].shape[2]
    cc = T.colour_channels(ch)
    code = Z.DTYPES[dtype]
    es = 1 if code == 0 else 4 if code == 1 else 2
    slot = H * W * ch * es
    fa, fb = Z.affine(8, SCALE, BIAS)
    arena, soff = bytearray(16), []
    for img, _, _, _ in files:
        arena += bytes(-len(arena) % 16)
        soff.append(len(arena))
        arena += np.ascontiguousarray(img).tobytes()
    a = np.frombuffer(bytes(arena), np.uint8).copy()  # exactly as long as the pixels
    luts = bytearray()
    hist_files = [i for i, f in enumerate(files) if f[1] in (T.AUTOCONTRAST, T.EQUALIZE)]
    order = hist_files + [i for i in range(len(files)) if i not in hist_files]
    tasks, n_hist_tasks = [], 0
    for i in order:
        img, op, param, user = files[i]
        lut_off = len(luts)
        luts += bytes(user) if op == T.TABLE else bytes(T.table(op, param) or 256) if i not in hist_files else bytes(256)
        for p0 in range(0, H * W, run_len):
            t = ToneTask(src_off=soff[i], out_off=GAP + i * slot, hist_off=(hist_files.index(i) if i in hist_files else 0) * cc * 1024,
                         lut_off=lut_off, pix0=p0, pix_n=min(run_len, H * W - p0), out_w=W, out_h=H, channels=ch, colour_channels=cc,
                         dtype=code, op=op)
            t.out_sx, t.out_sy, t.out_sc = (1, W, H * W) if layout == "chw" else (ch, W * ch, 1)
            t.a[:] = [float(v) for v in fa]
            t.b[:] = [float(v) for v in fb]
            tasks.append(t)
            n_hist_tasks += i in hist_files
    if spoil:
        spoil(tasks)
    n = len(tasks)
    arr = (ToneTask * n)(*tasks)
    hist = np.zeros((len(hist_files), cc, 256), np.uint32)
    la = np.frombuffer(bytes(luts), np.uint8).copy()
    out = np.full(GAP + len(files) * slot + GAP, FILL, np.uint8)
    assert launch("png_tone_hist", a, hist, arr, n_hist_tasks, grid, emu=_emu) == 0
    assert launch("png_tone_apply", a, out, arr, hist, la, n, grid, emu=_emu) == 0
    assert (out[:GAP] == FILL).all() and (out[GAP + len(files) * slot:] == FILL).all(), "the sentinel around the tensor was written"
    npdt = {0: np.uint8, 1: np.float32, 2: np.float16, 3: np.uint16}[code]
    shape = (len(files), ch, H, W) if layout == "chw" else (len(files), H, W, ch)
    return out[GAP: GAP + len(files) * slot].view(npdt).reshape(shape), hist, n


def _want(f, dtype, layout):
    img, op, param, user = f
    return T.tone(img, op, param, dtype, SCALE, BIAS, layout, user)


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
@pytest.mark.parametrize("size", SIZES)
def test_tone_kernels_against_the_reference(size, ch, layout):
    files = _files(size, ch)
    cc = T.colour_channels(ch)
    for dtype in DTYPES:
        got, hist, n = run(files, size, dtype, layout)
        assert n == len(files) * -(-size[0] * size[1] // RUN) and n >= 5 * len(files)
        hf = [f for f in files if f[1] in (T.AUTOCONTRAST, T.EQUALIZE)]
        for k, f in enumerate(hf):
            assert np.array_equal(hist[k], T.histogram(f[0], cc)), (k, "histogram")
        for i, f in enumerate(files):
            want = _want(f, dtype, layout)
            assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                (size, ch, layout, dtype, i, np.argwhere(got[i] != want)[:4])


def test_the_sources_take_every_path_of_the_rule():
    """the cases the parametrised test relies on are really there"""
    files = _files(SIZES[1], 3)
    cc = 3
    tabs = [T.tables(op, p, img, cc, u) for img, op, p, u in files]
    ident = np.arange(256, dtype=np.uint8)
    assert np.array_equal(tabs[2][0], ident) and np.array_equal(tabs[4][0], ident)  # a flat channel: the identity
    assert not np.array_equal(tabs[0][0], ident) and not np.array_equal(tabs[1][1], ident)
    assert tabs[3][0][255] == 255 and tabs[3][0][0] == 0 and tabs[9][0][255] == 255  # two values
    assert not np.array_equal(tabs[0], tabs[10]) and not np.array_equal(tabs[0][0], tabs[0][1])
    small = _files(SIZES[0], 1)  # 1273 pixels: step 4, entries reach the clamp
    h = T.histogram(small[0][0], 1)[0]
    assert (int(h.sum()) - int(h[np.nonzero(h)[0][-1]])) // 255 == 4


def test_rgb_runs_start_at_every_alignment():
    """a run length of 255 pixels: the first byte of an RGB run takes every residue mod 16"""
    size = SIZES[1]
    files = _files(size, 3)[:4]
    assert {(3 * p0) % 16 for p0 in range(0, size[0] * size[1], 255)} == set(range(16))
    got, hist, _ = run(files, size, "float32", "chw", run_len=255)
    for k, f in enumerate(files):
        assert np.array_equal(hist[k], T.histogram(f[0], 3))
        assert got[k].tobytes() == _want(f, "float32", "chw").tobytes()


def test_fewer_workgroups_than_tasks_and_long_runs():
    size = SIZES[1]
    files = _files(size, 4)
    want = [_want(f, "bfloat16", "hwc") for f in files]
    for run_len, grid in ((RUN, 3), (RUN, 1), (4096, 0), (4096, 2)):
        got, hist, _ = run(files, size, "bfloat16", "hwc", run_len=run_len, grid=grid)
        hf = [f for f in files if f[1] in (T.AUTOCONTRAST, T.EQUALIZE)]
        for k, f in enumerate(hf):
            assert np.array_equal(hist[k], T.histogram(f[0], 3)), (run_len, grid, k)
        for i in range(len(files)):
            assert got[i].tobytes() == want[i].tobytes(), (run_len, grid, i)


def test_tasks_that_break_a_bound_are_skipped():
    size = SIZES[0]
    files = _files(size, 3)
    per = -(-size[0] * size[1] // RUN)  # tasks per file; the order: the eight histogram files (0 1 2 3 4 6 9 10), then 5 7 8

    def spoil(tasks):
        for k in range(per):
            tasks[k].channels = 5                       # file 0
            tasks[per + k].hist_off += 4                # file 1
            tasks[2 * per + k].colour_channels = 2      # file 2
            tasks[3 * per + k].pix_n = 65537            # file 3
            tasks[4 * per + k].dtype = 4                # file 4
            tasks[5 * per + k].op = 6                   # file 6
            tasks[6 * per + k].pix0 = size[0] * size[1]  # file 9
            tasks[8 * per + k].lut_off += 8             # file 5
            tasks[9 * per + k].op = 0                   # file 7
        tasks[10 * per].out_w = 16385                   # file 8: its first run

    got, hist, _ = run(files, size, "uint", "hwc", spoil=spoil)
    for i in (0, 1, 2, 3, 4, 6, 9, 5, 7):
        assert (got[i] == FILL).all(), i
    assert not hist[:7].any() and np.array_equal(hist[7], T.histogram(files[10][0], 3))
    assert np.array_equal(got[10], _want(files[10], "uint", "hwc"))
    want8 = _want(files[8], "uint", "hwc").reshape(-1, 3)
    g8 = got[8].reshape(-1, 3)
    assert (g8[:RUN] == FILL).all() and np.array_equal(g8[RUN:], want8[RUN:])
