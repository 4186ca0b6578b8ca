"""The elastic deformation without a GPU (include/decode_png.h: debig_png_decode_batch_tensor_elastic, _labels_elastic,
_color_labels_elastic): the rule's properties on the numpy restatement tests/png_elastic_ref.py, the host's C helpers against it,
the displacement against float64 Catmull-Rom and torch.nn.functional.grid_sample, the quantiser's limits, every argument check of
the three C calls that is decided before a device is touched, the Python keywords and png_elastic_field."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_label_ref as CR  # noqa: E402
import png_elastic_ref as ER  # noqa: E402
import png_label_ref as LR  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_warp_ref as WR  # noqa: E402
import test_png_color_labels_cpu as CC  # noqa: E402  (the colour-label descriptors and their BAD_ARG cases)
import test_png_warp_cpu as TW  # noqa: E402  (the tensor / label descriptors of the warp calls)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_FORMAT = -2, -1
DUMMY, SENTINEL = TW.DUMMY, TW.SENTINEL
GRIDS = [(2, 2), (3, 5), (33, 33)]  # (grid_h, grid_w)
SIZES = [(1, 1), (33, 65), (64, 257)]  # (H, W)
ONE = 16384
LIMIT = 1 << 28


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
    L.debig_png_elastic_quantise.restype = C.c_int
    L.debig_png_elastic_quantise.argtypes = [C.POINTER(C.c_double), C.c_uint64, C.POINTER(C.c_int32)]
    L.debig_png_elastic_cell.restype = None
    L.debig_png_elastic_cell.argtypes = [C.c_uint32] * 3 + [C.POINTER(C.c_uint32)] * 2
    L.debig_png_elastic_weights.restype = None
    L.debig_png_elastic_weights.argtypes = [C.c_uint32, C.POINTER(C.c_int32)]
    L.debig_png_elastic_displacement.restype = C.c_int
    L.debig_png_elastic_displacement.argtypes = [C.POINTER(C.c_int32)] + [C.c_uint32] * 6 + [C.POINTER(C.c_int64)] * 2
    L.debig_png_decode_batch_tensor_elastic.restype = C.c_int
    L.debig_png_decode_batch_tensor_elastic.argtypes = [C.c_void_p] * 8 + [C.c_uint32] + [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
    L.debig_png_decode_batch_labels_elastic.restype = C.c_int
    L.debig_png_decode_batch_labels_elastic.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
    L.debig_png_decode_batch_color_labels_elastic.restype = C.c_int
    L.debig_png_decode_batch_color_labels_elastic.argtypes = [C.c_void_p] * 8 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
    return L


def _field(grid, seed, amp=3.0):
    return np.random.default_rng(seed).uniform(-amp, amp, size=grid + (2,))


# ---- the rule on the restatement -----------------------------------------------------------------------------------------------------

def test_weights_over_every_t():
    """the five facts the header states, over all 16385 values of t"""
    t = np.arange(ONE + 1)
    w = ER.weights(t)
    assert (w.sum(axis=0) == ONE).all()
    assert w[:, 0].tolist() == [0, ONE, 0, 0] and w[:, ONE].tolist() == [0, 0, ONE, 0]
    assert np.array_equal(w, w[::-1, ::-1])  # w_j(t) = w_(1-j)(16384 - t)
    assert int(np.abs(w).sum(axis=0).max()) <= 20480
    assert float(np.abs(w - ER.weights_float64(t)).max()) <= 1.5


def test_cells_and_fractions():
    for W in (1, 2, 3, 33, 65, 257, 4096, 16384):
        for g in (2, 3, 5, 9, 33):
            k, t = ER.cell(np.arange(W), W, g)  # (asserts k <= g - 2 and t in 0 .. 16384)
            p = (np.arange(W) + 0.5) * (g - 1) / W
            assert (np.abs(k + t / ONE - p) <= 2.0 ** -15 + 1e-12).all(), (W, g)
    k, t = ER.cell(np.arange(4), 4, 9)
    assert k.tolist() == [1, 3, 5, 7] and t.tolist() == [0] * 4  # (c): every pixel centre on a node


def test_properties_a_b_c_on_the_restatement():
    size = (33, 65)
    for M in ((1, 0, 0, 0, 1, 0), (0.75, -0.5, 3.25, 0.125, 1.5, -7.0), (-2, 0, 64, 0, -2, 30)):
        m = WR.quantise(M)
        for grid in GRIDS:
            # (a) no field, or a field of zeros: the affine positions
            for qf in (None, np.zeros(grid + (2,), np.int64)):
                assert all(np.array_equal(x, y) for x, y in zip(ER.positions(size, m, qf), WR.positions(size, m)))
            # (b) the same whole number of pixels at every node: the affine positions of the moved matrix
            for a, b in ((3, -2), (-4096, 4096), (1, 0)):
                const = np.broadcast_to(np.array([a << 16, b << 16]), grid + (2,))
                moved = list(m)
                moved[2] += a * m[0] + b * m[1]
                moved[5] += a * m[3] + b * m[4]
                if abs(moved[2]) <= 1 << 40 and abs(moved[5]) <= 1 << 40:
                    assert all(np.array_equal(x, y) for x, y in zip(ER.positions(size, m, const), WR.positions(size, moved))), (M, grid, a, b)
    # (c) where t = 0 on both axes D is the node's value: a 4 x 4 output under a 9 x 9 grid
    q9 = ER.quantise_field(_field((9, 9), 5, 4096.0))
    Dx, Dy = ER.displacement((4, 4), q9)
    assert np.array_equal(Dx, q9[1::2, 1::2, 0]) and np.array_equal(Dy, q9[1::2, 1::2, 1])
    # nodes at the limit everywhere: |S| stays below 2^57 (asserted inside) and |D| below 2^29
    worst = np.where(np.indices((33, 33)).sum(axis=0) % 2 == 0, LIMIT, -LIMIT)
    Dx, _ = ER.displacement((64, 257), np.stack([worst, -worst], axis=2))
    assert int(np.abs(Dx).max()) < 1 << 29


def _float64_bound(A):
    """see test_displacement_against_float64_catmull_rom"""
    return A * (10 * 2.0 ** -15 + 15 * 2.0 ** -14) + 2.5625 * 2.0 ** -17 + 1e-9 * (1.0 + A)


@pytest.mark.parametrize("amp", [3.0, 4096.0])
def test_displacement_against_float64_catmull_rom(amp):
    """D / 65536 against the Catmull-Rom interpolation of the UNQUANTISED field in float64 (exact cell and fraction), in output
    pixels.  The bound, with A the largest |node| in pixels, tau the exact fraction, w the real weights and w^ the integer ones:
      1. t is rem 2^14 / den rounded half up, so |t / 2^14 - tau| <= 2^-15 per axis.  The interpolant's derivative along an axis
         is sum_j w_j'(tau) (...); on [0, 1] the four |w_j'| are at most 1/2 (1 + 25/9 + 25/9 + 1) < 4 together, and the other
         axis contributes sum |w| <= 1.25 (the real weights at tau = 1/2: 2 (1/16 + 9/16)).  By the mean value theorem one axis
         moves the value by at most 2^-15 * 4 * 1.25 * A, both by 10 * 2^-15 * A;
      2. every integer weight lies within 1.5 * 2^-14 of w(t / 2^14) (test_weights_over_every_t), and sum |w^| <= 1.25:
         sum_ij |w^y_i w^x_j - wy_i wx_j| <= (4 * 1.5 * 2^-14) * 1.25 + 1.25 * (4 * 1.5 * 2^-14) = 15 * 2^-14, times A;
      3. a node is rounded to Q16: at most 2^-17 pixels, times sum |w^y| sum |w^x| <= 1.5625;
      4. D is S / 2^28 rounded: at most half a Q16 unit, 2^-17 pixels;
    and 10^-9 (1 + A) covers the float64 evaluation.  Together A (10 * 2^-15 + 15 * 2^-14) + 2.5625 * 2^-17: 0.0037 pixels for
    A = 3, and 5.0 pixels for nodes of 4096 pixels (a relative 0.0012)."""
    worst = 0.0
    for grid in GRIDS:
        for size in SIZES:
            F = _field(grid, 17 * grid[1] + size[1], amp)
            Dx, Dy = ER.displacement(size, ER.quantise_field(F))
            ref = ER.catmull_rom_float64(size, F)
            err = max(float(np.abs(Dx / 65536.0 - ref[:, :, 0]).max()), float(np.abs(Dy / 65536.0 - ref[:, :, 1]).max()))
            worst = max(worst, err)
            assert err <= _float64_bound(float(np.abs(F).max())), (grid, size, err)
    print(f"amp {amp}: largest difference to float64 Catmull-Rom {worst:.3g} pixels, bound {_float64_bound(amp):.3g}")


def test_a_smooth_image_against_grid_sample():
    """one smooth 8-bit image under a resize-to-fit matrix and a smooth field: the restatement (bilinear, UINT) against
    torch.nn.functional.grid_sample (float32, bilinear, zeros padding, align_corners=False) fed the float64 Catmull-Rom field.
    MEASURED largest difference: 1 eight-bit step (Q14 weights and a 16-bit intermediate row here, float32 arithmetic and one
    rounding there); asserted with a margin of one step over that."""
    import torch
    import torch.nn.functional as F_

    h, w, H, W = 48, 64, 40, 56
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([127.5 + 120 * np.sin(xx / 9.0) * np.cos(yy / 7.0), 127.5 + 120 * np.cos((xx + yy) / 11.0), 2.0 * xx + yy],
                   axis=2).round().astype(np.uint8)
    from debigulator_amd.api import png_elastic_field, png_warp_matrix

    M = png_warp_matrix((w, h), (H, W), scale=(W / w, H / h))  # resize to fit
    field = png_elastic_field((H, W), alpha=4.0, sigma=8.0, rng=3)
    got = ER.warp(img, (H, W), WR.quantise([v for r in M for v in r]), ER.quantise_field(field), WR.BILINEAR, "uint", WR.CONSTANT)
    disp = ER.catmull_rom_float64((H, W), field)
    X = np.arange(W)[None, :] + 0.5 + disp[:, :, 0]
    Y = np.arange(H)[:, None] + 0.5 + disp[:, :, 1]
    grid = np.stack([2.0 * X / W - 1.0, 2.0 * Y / H - 1.0], axis=2)  # (the fit matrix scales by w / W: normalised, it drops out)
    ref = F_.grid_sample(torch.from_numpy(img.astype(np.float32)).permute(2, 0, 1)[None], torch.from_numpy(grid.astype(np.float32))[None],
                         mode="bilinear", padding_mode="zeros", align_corners=False)[0].permute(1, 2, 0).numpy()
    diff = int(np.abs(got.astype(np.int64) - np.floor(ref.astype(np.float64) + 0.5).astype(np.int64)).max())
    print("largest difference to grid_sample:", diff)
    assert diff <= 2


# ---- the host helpers against the restatement -------------------------------------------------------------------------------------

def test_host_weights_and_cells_against_the_restatement(lib):
    w = (C.c_int32 * 4)()
    want = ER.weights(np.arange(ONE + 1))
    for t in range(ONE + 1):
        lib.debig_png_elastic_weights(t, w)
        assert list(w) == want[:, t].tolist(), t
    k, t = C.c_uint32(), C.c_uint32()
    for W in (1, 33, 65, 257, 16384):
        for g in (2, 3, 5, 33):
            wk, wt = ER.cell(np.arange(W), W, g)
            for X in (range(W) if W <= 257 else (0, 1, 8191, 8192, 16382, 16383)):
                lib.debig_png_elastic_cell(X, W, g, C.byref(k), C.byref(t))
                assert (k.value, t.value) == (int(wk[X]), int(wt[X])), (W, g, X)


def _host_displacement(lib, q, size):
    H, W = size
    gh, gw = q.shape[:2]
    q32 = np.ascontiguousarray(q, dtype=np.int32)
    Dx, Dy = np.zeros(size, np.int64), np.zeros(size, np.int64)
    a, b = C.c_int64(), C.c_int64()
    for Y in range(H):
        for X in range(W):
            assert lib.debig_png_elastic_displacement(q32.ctypes.data_as(C.POINTER(C.c_int32)), gw, gh, W, H, X, Y, C.byref(a), C.byref(b)) == 1
            Dx[Y, X], Dy[Y, X] = a.value, b.value
    return Dx, Dy


@pytest.mark.parametrize("grid", GRIDS)
def test_host_displacement_against_the_restatement(lib, grid):
    """2 x 2, 3 x 5 and 33 x 33 nodes on outputs of 1 x 1 (more cells than pixels), 33 x 65 and 64 x 257; nodes up to the limit"""
    for size in SIZES:
        for kind in range(2):
            q = ER.quantise_field(_field(grid, size[1] + kind, 4096.0 if kind else 5.0))
            if kind:
                q[0, 0], q[-1, -1] = (LIMIT, -LIMIT), (-LIMIT, LIMIT)
            got, want = _host_displacement(lib, q, size), ER.displacement(size, q)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (grid, size, kind)
    q = np.zeros((3, 5, 2), np.int32)
    a, b = C.c_int64(), C.c_int64()
    ptr = q.ctypes.data_as(C.POINTER(C.c_int32))
    for gw, gh, W, H, X, Y in ((1, 3, 8, 8, 0, 0), (5, 34, 8, 8, 0, 0), (5, 3, 0, 8, 0, 0), (5, 3, 8, 16385, 0, 0), (5, 3, 8, 8, 8, 0),
                               (5, 3, 8, 8, 0, 8)):
        assert lib.debig_png_elastic_displacement(ptr, gw, gh, W, H, X, Y, C.byref(a), C.byref(b)) == 0
    assert lib.debig_png_elastic_displacement(None, 5, 3, 8, 8, 0, 0, C.byref(a), C.byref(b)) == 0
    q[1, 2, 0] = LIMIT + 1  # a node beyond the limit among the sixteen
    assert lib.debig_png_elastic_displacement(ptr, 5, 3, 8, 8, 4, 4, C.byref(a), C.byref(b)) == 0


def _host_q(lib, v):
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    q = np.zeros(v.size, np.int32)
    ok = lib.debig_png_elastic_quantise(v.ctypes.data_as(C.POINTER(C.c_double)), v.size, q.ctypes.data_as(C.POINTER(C.c_int32)))
    return q.tolist() if ok else None


def test_quantise_against_the_restatement_and_at_its_limits(lib):
    rng = np.random.default_rng(2)
    for k in range(50):
        F = rng.uniform(-4096, 4096, size=(3, 4, 2)) * 10.0 ** -rng.integers(0, 6)
        if k % 5 == 0:
            F[0, 0, 0] = (int(rng.integers(-1000, 1000)) + 0.5) / 65536.0  # an exact half of a Q16 unit
        assert _host_q(lib, F) == ER.quantise_field(F).reshape(-1).tolist()
    assert _host_q(lib, [0.5 / 65536, -0.5 / 65536, 1.5 / 65536, -1.5 / 65536, 0.49999 / 65536, -0.49999 / 65536]) == [1, -1, 2, -2, 0, 0]
    assert _host_q(lib, [4096.0, -4096.0, 0.0, -0.0]) == [LIMIT, -LIMIT, 0, 0]
    for bad in (math.nextafter(4096.0, math.inf), -math.nextafter(4096.0, math.inf), 4097.0, math.inf, -math.inf, math.nan):
        assert _host_q(lib, [0.0, bad]) is None and ER.quantise_field(np.array([[[0.0, bad]]])) is None, bad
    assert _host_q(lib, [math.nextafter(4096.0, 0.0)]) == [LIMIT]  # (rounds to the limit itself)
    assert _host_q(lib, []) == []


# ---- the three C calls: what needs no device ------------------------------------------------------------------------------------------

def _elastics(api, n, fields, grid=(3, 5)):
    """fields: "zeros" | None | a list of arrays / None -> (PngElastic * n or None, the arrays kept alive)"""
    if fields is None:
        return None, []
    arrs = [np.zeros(grid + (2,)) for _ in range(n)] if fields == "zeros" else \
        [None if f is None else np.ascontiguousarray(f, dtype=np.float64) for f in fields]
    es = (api.PngElastic * n)()
    for i, a in enumerate(arrs):
        es[i].nodes = None if a is None else a.ctypes.data
    return es, arrs


def _edesc(api, gw=5, gh=3, r0=0, r1=0):
    return api.PngElasticDesc(gw, gh, (C.c_uint32 * 2)(r0, r1))


def _tensor_call(lib, api, files, desc, wd, out=DUMMY, boxes=None, warps="ident", fields="zeros", ed="good", colors=None, tones=None,
                 tables=None, n_tables=0, blurs=None):
    n = len(files)
    ins, sizes, st, bx, ws = TW._files(files, boxes, [TW.IDENT] * n if warps == "ident" else warps)
    es, keep = _elastics(api, n, fields)
    ed = _edesc(api) if ed == "good" else ed
    rc = lib.debig_png_decode_batch_tensor_elastic(ins, sizes, out, bx, ws, colors, tones, tables, n_tables, blurs, st, None, n, 0,
                                                   C.byref(desc) if desc is not None else None, C.byref(wd) if wd is not None else None,
                                                   es, C.byref(ed) if ed is not None else None)
    return rc, list(st)


def _label_call(lib, api, files, desc, wd, out=DUMMY, boxes=None, warps="ident", fields="zeros", ed="good"):
    n = len(files)
    ins, sizes, st, bx, ws = TW._files(files, boxes, [TW.IDENT] * n if warps == "ident" else warps)
    es, keep = _elastics(api, n, fields)
    ed = _edesc(api) if ed == "good" else ed
    rc = lib.debig_png_decode_batch_labels_elastic(ins, sizes, out, bx, ws, st, None, n, 0, C.byref(desc) if desc is not None else None,
                                                   C.byref(wd) if wd is not None else None, es, C.byref(ed) if ed is not None else None)
    return rc, list(st)


def _clbl_call(lib, api, files, desc, wd, out=DUMMY, boxes=None, warps="ident", fields="zeros", ed="good"):
    n = len(files)
    ins, sizes, st, bx, ws = TW._files(files, boxes, [TW.IDENT] * n if warps == "ident" else warps)
    um = (C.c_uint32 * n)(*[SENTINEL] * n)
    es, keep = _elastics(api, n, fields)
    ed = _edesc(api) if ed == "good" else ed
    rc = lib.debig_png_decode_batch_color_labels_elastic(ins, sizes, out, bx, ws, st, None, um, n, 0,
                                                         C.byref(desc) if desc is not None else None,
                                                         C.byref(wd) if wd is not None else None, es, C.byref(ed) if ed is not None else None)
    return rc, list(st), list(um)


def _bad_descs(api):
    return [None, _edesc(api, gw=1), _edesc(api, gh=1), _edesc(api, gw=34), _edesc(api, gh=34), _edesc(api, gw=0, gh=0),
            _edesc(api, r0=1), _edesc(api, r1=1)]


def test_tensor_argument_checks_leave_status_unwritten(lib, api):
    """every BAD_ARG path of the affine calls it stands for, then the elastic arguments', before any file is read"""
    f = [b"not a png"]
    td, wd = TW._tdesc, TW._wdesc
    bad = [(td(api), wd(api, filter=TW.BICUBIC)), (td(api), wd(api, filter=3)), (td(api), wd(api, alpha_mode=1)), (td(api), wd(api, alpha_mode=2)),
           (td(api), wd(api, border_mode=2)), (td(api), wd(api, reserved=1)), (td(api, flags=1), wd(api)),
           (td(api), wd(api, border=(0, 0, 256, 0))), (td(api, fmt=TW.GRAY), wd(api, border=(256, 0, 0, 0))), (td(api), None),
           (None, wd(api)), (td(api, w=0), wd(api)), (td(api, dtype=4), wd(api))]
    cs = (api.PngColor * 1)()
    ts = (api.PngTone * 1)()
    bs = (api.PngBlur * 1)()
    for extra in (dict(), dict(colors=cs), dict(tones=ts), dict(blurs=bs), dict(colors=cs, tones=ts, blurs=bs)):
        for desc, w in bad:
            assert _tensor_call(lib, api, f, desc, w, **extra) == (BAD_ARG, [SENTINEL]), (desc, w, list(extra))
        assert _tensor_call(lib, api, f, td(api), wd(api), warps=None, **extra) == (BAD_ARG, [SENTINEL])  # the matrices are required
        assert _tensor_call(lib, api, f, td(api), None, warps=None, **extra) == (BAD_ARG, [SENTINEL]), list(extra)
        assert _tensor_call(lib, api, f, td(api), wd(api), out=DUMMY + 8, **extra) == (BAD_ARG, [SENTINEL])
        assert _tensor_call(lib, api, f, td(api, fmt=4), wd(api), **extra) == (BAD_FORMAT, [SENTINEL])
        # the elastic arguments
        assert _tensor_call(lib, api, f, td(api), wd(api), fields=None, **extra) == (BAD_ARG, [SENTINEL]), list(extra)
        for ed in _bad_descs(api):
            assert _tensor_call(lib, api, f, td(api), wd(api), ed=ed, **extra) == (BAD_ARG, [SENTINEL]), (ed, list(extra))
        # at the edge of their ranges they pass, a file without a field included, and the file is reached
        for ed in (_edesc(api, 2, 2), _edesc(api, 33, 33), _edesc(api, 2, 33)):
            assert _tensor_call(lib, api, f, td(api), wd(api), ed=ed, fields=[None], **extra) == (0, [R.E_SIGNATURE]), list(extra)
        assert _tensor_call(lib, api, f, td(api), wd(api), **extra) == (0, [R.E_SIGNATURE]), list(extra)
    assert _tensor_call(lib, api, f, td(api, fmt=TW.GRAY), wd(api), colors=cs) == (BAD_ARG, [SENTINEL])
    for extra in (dict(tones=ts), dict(blurs=bs)):
        assert _tensor_call(lib, api, f, td(api, fmt=TW.RGB | TW.D16), wd(api, border=(0, 0, 0, 0)), **extra) == (BAD_ARG, [SENTINEL])
        assert _tensor_call(lib, api, f, td(api), wd(api), n_tables=1, **extra) == (BAD_ARG, [SENTINEL])
    assert lib.debig_png_decode_batch_tensor_elastic(None, None, None, None, None, None, None, None, 0, None, None, None, 0, 0, None, None,
                                                     None, None) == 0


def test_label_argument_checks_leave_status_unwritten(lib, api):
    f = [b"not a png"]
    LD, LW = api.PngLabelDesc, api.PngLabelWarpDesc
    U8, U16, I32, I64 = range(4)
    bad = [(LD(out_w=8, out_h=6, dtype=U8), LW(0, 256)), (LD(out_w=8, out_h=6, dtype=U8), LW(0, -1)),
           (LD(out_w=8, out_h=6, dtype=U16), LW(0, 65536)), (LD(out_w=8, out_h=6, dtype=I64), LW(2, 0)),
           (LD(out_w=8, out_h=6, dtype=I64), None), (None, LW(0, 0)), (LD(out_w=0, out_h=6, dtype=I64), LW(0, 0)),
           (LD(out_w=8, out_h=6, dtype=4), LW(0, 0)), (LD(out_w=8, out_h=6, dtype=I32, reserved=1), LW(0, 0))]
    for desc, wd in bad:
        assert _label_call(lib, api, f, desc, wd) == (BAD_ARG, [SENTINEL]), (desc, wd)
    good = LD(out_w=8, out_h=6, dtype=I64), LW(0, 0)
    assert _label_call(lib, api, f, *good, warps=None) == (BAD_ARG, [SENTINEL])
    assert _label_call(lib, api, f, *good, fields=None) == (BAD_ARG, [SENTINEL])
    for ed in _bad_descs(api):
        assert _label_call(lib, api, f, *good, ed=ed) == (BAD_ARG, [SENTINEL]), ed
    assert lib.debig_png_decode_batch_labels_elastic(None, None, None, None, None, None, None, 0, 0, None, None, None, None) == 0
    for desc, wd in ((LD(out_w=8, out_h=6, dtype=U8), LW(0, 255)), (LD(out_w=8, out_h=6, dtype=I32), LW(0, -1)), good):
        assert _label_call(lib, api, f, desc, wd, fields=[None]) == (0, [R.E_SIGNATURE])


def test_color_label_argument_checks_leave_status_and_unmatched_unwritten(lib, api):
    f = [b"not a png", b"x"]
    untouched = (BAD_ARG, [SENTINEL] * 2, [SENTINEL] * 2)
    LW = api.PngLabelWarpDesc
    pack = CC._desc()
    u8 = CC._desc(dtype=0, mode=1, missing=0, maps=[CC._map([1, 2, 3])])
    assert _clbl_call(lib, api, f, pack, LW(0, 0), warps=None) == untouched
    assert _clbl_call(lib, api, f, pack, None) == untouched
    assert _clbl_call(lib, api, f, pack, LW(2, 0)) == untouched
    assert _clbl_call(lib, api, f, u8, LW(0, 256)) == untouched
    assert _clbl_call(lib, api, f, pack, LW(0, 0), fields=None) == untouched
    for ed in _bad_descs(api):
        assert _clbl_call(lib, api, f, pack, LW(0, 0), ed=ed) == untouched, ed
    for name, desc, off in CC.bad_arg_cases(2):  # every inherited check
        assert _clbl_call(lib, api, f, desc, LW(0, 0), None if off is None else DUMMY + off) == untouched, name
    assert _clbl_call(lib, api, f, u8, LW(1, 256), fields=[None, None]) == (0, [R.E_SIGNATURE] * 2, [0, 0])
    assert lib.debig_png_decode_batch_color_labels_elastic(None, None, None, None, None, None, None, None, 0, 0, None, None, None, None) == 0


def test_warp_status_is_decided_on_the_host_behind_label_and_box(lib, api):
    """E_LABEL, then E_BOX, then E_WARP -- a non-finite node, a node of 4097 pixels, a bad matrix under a good field --, each ahead
    of what the file holds later"""
    rng = np.random.default_rng(4)
    rgb = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    g8 = R.encode(R.random_image(rng, 9, 7, 0, 8), 0, 8)
    g8_crc = bytearray(g8)
    g8_crc[-20] ^= 1
    grid = (3, 5)
    ok = _field(grid, 1)
    nan, big, edge = ok.copy(), ok.copy(), ok.copy()
    nan[2, 4, 1] = math.nan
    big[0, 0, 0] = -4097.0
    edge[1, 1] = (4096.0, -4096.0)
    L, B, Wp = LR.E_LABEL, LR.E_BOX, WR.E_WARP
    # E_LABEL > E_BOX (file 0), E_LABEL > E_WARP (1), E_BOX > E_WARP (2), E_WARP > CRC (3), E_WARP > missing IDAT (4), E_WARP by the
    # matrix under a good field (5); a walk error before the end of IHDR stands (6, 7), also under fields that are fine
    files = [rgb, rgb, g8, bytes(g8_crc), g8[:40], g8, g8[:30], b"\x89PNG"]
    boxes = [(0, 0, 10, 1), None, (0, 0, 10, 1), None, None, None, None, None]
    fields = [nan, nan, big, nan, big, ok, edge, None]
    warps = [TW.IDENT] * 5 + [(1, 32768.5, 0, 0, 1, 0)] + [TW.IDENT] * 2
    ld = api.PngLabelDesc(out_w=8, out_h=6, dtype=3)
    rc, st = _label_call(lib, api, files, ld, api.PngLabelWarpDesc(0, -1), boxes=boxes, warps=warps, fields=fields)
    assert (rc, st) == (0, [L, L, B, Wp, Wp, Wp, R.E_CHUNK, R.E_SIGNATURE])
    for extra in (dict(), dict(blurs=(api.PngBlur * 8)()), dict(tones=(api.PngTone * 8)(), colors=(api.PngColor * 8)())):
        rc, st = _tensor_call(lib, api, files, TW._tdesc(api), TW._wdesc(api), boxes=boxes, warps=warps, fields=fields, **extra)
        assert (rc, st) == (0, [B, Wp, B, Wp, Wp, Wp, R.E_CHUNK, R.E_SIGNATURE]), list(extra)
    rgb16 = R.encode(R.random_image(rng, 9, 7, 2, 16), 2, 16)
    rc, st, um = _clbl_call(lib, api, [rgb16, rgb, rgb, rgb[:40]], CC._desc(), api.PngLabelWarpDesc(0, 0),
                            boxes=[None, (3, 3, 0, 2), None, None], fields=[nan, big, big, nan])
    assert (rc, st, um) == (0, [CR.E_LABEL, CR.E_BOX, Wp, Wp], [0] * 4)


# ---- Python ------------------------------------------------------------------------------------------------------------------------------

def test_python_keywords(api):
    import inspect

    for fn in (api.png_decode_batch_tensor, api.png_decode_batch_labels, api.png_decode_batch_color_labels):
        assert inspect.signature(fn).parameters["elastic"].default is None
    assert C.sizeof(api.PngElastic) == 8 and C.sizeof(api.PngElasticDesc) == 16
    z = np.zeros((3, 5, 2))
    for fn in (api.png_decode_batch_tensor, api.png_decode_batch_labels, api.png_decode_batch_color_labels):
        with pytest.raises(ValueError, match="exclude"):
            fn([b""], (4, 4), elastic=[z], perspective=[None])
        with pytest.raises(ValueError, match="one entry"):
            fn([b""], (4, 4), elastic=[z, z])
        with pytest.raises(ValueError, match="one grid size"):
            fn([b"", b"", b""], (4, 4), elastic=[z, None, np.zeros((5, 3, 2))])
        for bad in (np.zeros((3, 5)), np.zeros((3, 5, 3)), np.zeros((1, 5, 2)), np.zeros((3, 34, 2)), np.zeros((2,))):
            with pytest.raises(ValueError, match="grid_h, grid_w, 2"):
                fn([b""], (4, 4), elastic=[bad])
        with pytest.raises(ValueError, match="boxes"):
            fn([b""], (4, 4), elastic=[z], boxes=[None, None])
    # the rules of the warp descriptors hold under a field as well, with and without warp=
    for kw in (dict(filter="bicubic"), dict(alpha="over"), dict(border="wrap"), dict(border="clamp", border_value=0.5)):
        for w in (dict(), dict(warp=[None])):
            with pytest.raises(ValueError):
                api.png_decode_batch_tensor([b""], (4, 4), elastic=[z], **kw, **w)
    for fn in (api.png_decode_batch_labels, api.png_decode_batch_color_labels):
        for kw in (dict(border="mirror"), dict(border="clamp", border_label=3), dict(border_label=2 ** 31)):
            with pytest.raises(ValueError):
                fn([b""], (4, 4), elastic=[z], **kw)
    es, ed = api._png_elastics([None, z, None], 3)
    assert (ed.grid_w, ed.grid_h, list(ed.reserved)) == (5, 3, [0, 0]) and es[0].nodes is None and es[1].nodes and es[2].nodes is None
    es, ed = api._png_elastics([None], 1)
    assert (ed.grid_w, ed.grid_h) == (2, 2) and es[0].nodes is None  # (no field at all: any legal grid)


def test_fit_matrices_without_warp(api):
    """without warp= a file takes png_warp_matrix((crop_w, crop_h), size); an unreadable header takes the identity"""
    rng = np.random.default_rng(8)
    png = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    ws = api._png_fit_warps([png, png, png, b"junk"], [None, (1, 2, 4, 3), (0, 0, 0, 0), None], (6, 8))
    assert ws[0] == api.png_warp_matrix((9, 7), (6, 8)) == ws[2] and ws[1] == api.png_warp_matrix((4, 3), (6, 8)) and ws[3] is None
    assert api._png_fit_warps([png], None, (7, 9)) == [((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))]


def test_png_elastic_field(api):
    f = api.png_elastic_field((64, 96), alpha=5.0, sigma=8.0, rng=1)
    assert f.shape == (9, 13, 2) and f.dtype == np.float64  # the default grid: a node spacing of about sigma
    assert np.array_equal(f, api.png_elastic_field((64, 96), alpha=5.0, sigma=8.0, rng=1))
    assert np.array_equal(f, api.png_elastic_field((64, 96), alpha=5.0, sigma=8.0, rng=np.random.default_rng(1)))
    assert not np.array_equal(f, api.png_elastic_field((64, 96), alpha=5.0, sigma=8.0, rng=2))
    assert 0.0 < float(np.abs(f).max()) <= 5.0  # smoothing is a convex combination of noise in [-1, 1]
    assert api.png_elastic_field((1, 1), 1.0, 50.0).shape == (2, 2, 2) and api.png_elastic_field((2000, 3000), 1.0, 4.0, rng=0).shape == (33, 33, 2)
    g = api.png_elastic_field((64, 96), alpha=(1e6, 2.0), sigma=1.0, grid=(3, 33), rng=5)
    assert g.shape == (3, 33, 2) and float(np.abs(g[:, :, 0]).max()) == 4096.0 and float(np.abs(g[:, :, 1]).max()) <= 2.0
    assert ER.quantise_field(g) is not None
    # smoother with a larger sigma: neighbouring nodes differ less
    rough = api.png_elastic_field((64, 64), 1.0, 2.0, grid=(33, 33), rng=3)
    soft = api.png_elastic_field((64, 64), 1.0, 12.0, grid=(33, 33), rng=3)
    assert np.abs(np.diff(soft, axis=1)).mean() < 0.25 * np.abs(np.diff(rough, axis=1)).mean()
    for bad in (dict(size=(0, 4), alpha=1, sigma=1), dict(size=(4, 4), alpha=1, sigma=0), dict(size=(4, 4), alpha=1, sigma=1, grid=(1, 5)),
                dict(size=(4, 4), alpha=1, sigma=1, grid=(5, 34))):
        with pytest.raises(ValueError):
            api.png_elastic_field(**bad)


def test_symbols_are_exported(lib):
    for name in ("debig_png_elastic_quantise", "debig_png_elastic_cell", "debig_png_elastic_weights", "debig_png_elastic_displacement",
                 "debig_png_decode_batch_tensor_elastic", "debig_png_decode_batch_labels_elastic",
                 "debig_png_decode_batch_color_labels_elastic", "debig_hip_png_elastic_batch", "debig_hip_png_elastic_color_batch",
                 "debig_hip_png_label_elastic_batch", "debig_hip_png_color_label_elastic_batch"):
        assert hasattr(lib, name), name


# ---- the sanitizer programs (stand-alone, plain child processes) ---------------------------------------------------------------------

@pytest.mark.parametrize("script", ["asan_png_elastic.sh", "asan_png_elastic_emu.sh"])
def test_stand_alone_programs_under_address_and_undefined_sanitizers(script, tmp_path):
    r = subprocess.run(["sh", os.path.join(ROOT, "tools", script), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
