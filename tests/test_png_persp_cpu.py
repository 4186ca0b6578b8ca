"""The perspective warp without a GPU (include/decode_png.h: debig_png_decode_batch_tensor_persp, _labels_persp, _color_labels_persp):
the restatement tests/png_persp_ref.py against its own consequences, against Pillow and against float64; the host's quantiser and
range check against the restatement; what the three C calls decide on the host alone -- every argument check (status left at its
sentinel) and E_WARP with its place in the order of statuses --; api.png_perspective_matrix and the Python keywords' refusals; and
the two stand-alone sanitizer programs of tools/ (host layer; emulated kernels), built and run as plain child processes."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_label_ref as CR  # noqa: E402
import png_label_ref as LR  # noqa: E402
import png_persp_ref as PR  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_warp_ref as WR  # noqa: E402
import test_png_color_labels_cpu as CC  # noqa: E402  (the colour-label descriptors and their BAD_ARG cases)
import test_png_warp_cpu as TW  # noqa: E402  (the tensor / label descriptors of the warp calls)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_FORMAT = -2, -1
DUMMY, SENTINEL = TW.DUMMY, TW.SENTINEL
IDENT9 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
ONE = 1 << 30


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
    L.debig_png_persp_quantise.restype = C.c_int
    L.debig_png_persp_quantise.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.debig_png_persp_range.restype = C.c_int
    L.debig_png_persp_range.argtypes = [C.POINTER(C.c_int64), C.c_uint32, C.c_uint32]
    L.debig_png_decode_batch_tensor_persp.restype = C.c_int
    L.debig_png_decode_batch_tensor_persp.argtypes = [C.c_void_p] * 8 + [C.c_uint32] + [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 2
    L.debig_png_decode_batch_labels_persp.restype = C.c_int
    L.debig_png_decode_batch_labels_persp.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.debig_png_decode_batch_color_labels_persp.restype = C.c_int
    L.debig_png_decode_batch_color_labels_persp.argtypes = [C.c_void_p] * 8 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


# ---- the matrices of this file ---------------------------------------------------------------------------------------------------

def _quads(n, seed, max_crop=80, max_out=70):
    """n small random quadrilaterals: (crop (w, h), output (H, W), the 3 x 3 inverse matrix in float64, its nine integers)"""
    from debigulator_amd.api import png_perspective_matrix

    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        cw, chh = (int(v) for v in rng.integers(8, max_crop + 1, 2))
        H, W = (int(v) for v in rng.integers(6, max_out + 1, 2))
        quad = np.array([(0, 0), (cw, 0), (cw, chh), (0, chh)], np.float64) + rng.uniform(-0.3, 0.3, (4, 2)) * (cw, chh)
        M = png_perspective_matrix(quad, (H, W))
        m = PR.quantise([v for r in M for v in r])
        if m is not None and PR.range_ok(m, (H, W)):
            out.append(((cw, chh), (H, W), M, m))
    return out


def _corner_cases(W, H):
    """(m, accepted, (cx, cy), d): D == d at ONE corner pixel -- d a limit (accepted) or one beyond it (refused) -- while the other
    three corners lie inside the range and every |p_k| <= 2^32: that corner alone decides.  (2^33 at pixel (0, 0) with smaller
    values elsewhere would need p2 > 2^32: the one combination that does not exist.)"""
    corners = [(1, 1), (2 * W - 1, 1), (1, 2 * H - 1), (2 * W - 1, 2 * H - 1)]
    for at in corners:
        for lim, step in ((PR.D_MIN, -1), (PR.D_MAX, 1)):
            for d in (lim, lim + step):
                for p0, p1 in ((a, b) for a in range(-2, 3) for b in range(-2, 3)):
                    rest = d - p0 * at[0] - p1 * at[1]
                    if rest % 2 or abs(rest // 2) > 1 << 32:
                        continue
                    if all(PR.D_MIN <= p0 * cx + p1 * cy + rest <= PR.D_MAX for cx, cy in corners if (cx, cy) != at):
                        yield [0] * 6 + [p0, p1, rest // 2], d == lim, at, d
                        break


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def test_row_2_of_the_identity_gives_the_affine_positions_exactly():
    from debigulator_amd.api import png_warp_matrix

    rng = np.random.default_rng(20)
    for k in range(20):
        w, h, H, W = (int(v) for v in rng.integers(1, 90, 4))
        M = png_warp_matrix((w, h), (H, W), angle=float(rng.uniform(-180, 180)), scale=float(rng.uniform(0.3, 3)),
                            shear=(float(rng.uniform(-20, 20)), 0), translate=(float(rng.uniform(-9, 9)), float(rng.uniform(-9, 9))))
        m = PR.quantise([v for r in M for v in r] + [0, 0, 1])
        assert m[:6] == WR.quantise([v for r in M for v in r]) and m[6:] == [0, 0, ONE]
        _, _, D = PR.parts((H, W), m)
        assert (D == 1 << 31).all()
        for a, b in zip(PR.positions((H, W), m), WR.positions((H, W), m[:6])):
            assert np.array_equal(a, b)


def test_scaling_the_whole_matrix_changes_no_position_and_the_two_step_division_is_the_wide_one():
    negative_with_remainder = 0
    for (cw, chh), size, _, m in _quads(40, 1):
        even = [v // 4 * 2 for v in m]
        base = PR.positions(size, even)
        for other in ([2 * v for v in even], [v // 2 for v in even]):
            assert PR.range_ok(other, size)
            assert all(np.array_equal(a, b) for a, b in zip(PR.positions(size, other), base))
        # a translation that takes part of the output to negative crop coordinates: floor and truncation differ there
        shifted = list(m)
        shifted[2] -= (cw // 2) << 16
        shifted[5] -= (chh // 3) << 16
        for mm in (m, shifted):
            NU, NV, D = PR.parts(size, mm)
            negative_with_remainder += int(((NU < 0) & (NU % D != 0)).sum() + ((NV < 0) & (NV % D != 0)).sum())
            for got, wide in zip(PR.positions(size, mm), PR.positions_wide(size, mm)):
                assert (got.astype(object) == wide).all()
    assert negative_with_remainder > 1000  # (truncation instead of floor does not pass the line above)
    t = np.frompyfunc(lambda n, d: -((-int(n) << 31) // int(d)) if n < 0 else (int(n) << 31) // int(d), 2, 1)  # the truncating form
    NU, _, D = PR.parts(size, shifted)
    assert (t(NU, D) != PR.positions_wide(size, shifted)[0]).any()


def test_quantise_and_range_of_the_restatement():
    assert PR.quantise(IDENT9) == [65536, 0, 0, 0, 65536, 0, 0, 0, ONE]
    assert PR.quantise([0] * 6 + [4.0, -4.0, 0.5 / ONE]) == [0] * 6 + [1 << 32, -(1 << 32), 1]  # the limit; a half goes away from zero
    assert PR.quantise([0] * 6 + [-0.5 / ONE, 1.5 / ONE, -1.5 / ONE]) == [0] * 6 + [-1, 2, -2]
    for bad in (math.nan, math.inf, -math.inf, math.nextafter(4.0, 5.0), -math.nextafter(4.0, 5.0)):
        for k in (6, 7, 8):
            M = list(IDENT9)
            M[k] = bad
            assert PR.quantise(M) is None, (k, bad)
    assert PR.quantise([1, 32768.5, 0, 0, 1, 0, 0, 0, 1]) is None  # rows 0 and 1: the affine limits
    # D is exactly the limit at a corner: accepted; one beyond: refused -- on each of the four corners
    W, H = 9, 5
    n = {True: 0, False: 0}
    for m, want, at, d in _corner_cases(W, H):
        assert PR.range_ok(m, (H, W)) == want, (m, at, d)
        assert int(PR.parts((H, W), m)[2][(at[1] - 1) // 2, (at[0] - 1) // 2]) == d
        n[want] += 1
    assert n[True] == 8 and n[False] >= 7, n
    assert not PR.range_ok([0] * 6 + [(1 << 32) + 1, 0, -(1 << 31)], (H, W))


@pytest.mark.parametrize("P", [8, 16])
def test_float64_bound_holds(P):
    """the integer rule (UINT, bilinear) against floor(float64 + 1/2) at the exact position: the bound of the docstring"""
    M = (1 << P) - 1
    assert PR.float64_bound(P) == math.floor(1 + M / 16384 + 2.0 ** (P - 17) + 2 * M / 131072 + 1e-6) == (1 if P == 8 else 6)
    assert PR.float64_bound(P) >= WR.float64_bound(P)
    rng = np.random.default_rng(P)
    worst = 0
    for (cw, chh), size, _, m in _quads(12, 2, 40, 40):
        src = rng.integers(0, 1 << P, size=(chh, cw, 2)).astype(np.uint8 if P == 8 else np.uint16)
        src[::3] = M  # full-scale steps
        src[::3, ::2] = 0
        for mode in (PR.CONSTANT, PR.CLAMP):
            got = PR.warp(src, size, m, PR.BILINEAR, "uint", mode, (M, 0, 0, 0)).astype(np.int64)
            ref = np.floor(PR.warp_float64(src, size, m, mode, (M, 0, 0, 0)) + 0.5).astype(np.int64)
            worst = max(worst, int(np.abs(got - ref).max()))
    print(f"P = {P}: largest difference {worst}, bound {PR.float64_bound(P)}")
    assert worst <= PR.float64_bound(P)


def test_nearest_pick_against_pillow():
    """Image.transform(size, PERSPECTIVE, coeffs, NEAREST) on the UNQUANTISED coefficients: at most 0.2 % of all elements differ
    (Q16 / Q30 quantisation next to ties)"""
    from PIL import Image

    rng = np.random.default_rng(7)
    differ = total = 0
    for (cw, chh), (H, W), M, m in _quads(40, 7):
        lab = rng.integers(1, 256, size=(chh, cw)).astype(np.uint8)  # (0 is Pillow's fill outside the image)
        flat = [v for r in M for v in r]
        assert flat[8] == 1.0
        pil = np.asarray(Image.fromarray(lab).transform((W, H), Image.PERSPECTIVE, flat[:8], Image.NEAREST))
        ours = PR.warp_labels(lab, (H, W), m, PR.CONSTANT, 0, None, None, "uint8")
        differ += int((pil != ours).sum())
        total += pil.size
    print(f"{differ} of {total} elements differ from Pillow ({100.0 * differ / total:.3f} %)")
    assert total > 40000 and differ <= 0.002 * total


# ---- the host: quantise and range ----------------------------------------------------------------------------------------------------

def _host_q(lib, M):
    m = (C.c_int64 * 9)(*[SENTINEL] * 9)
    return list(m) if lib.debig_png_persp_quantise((C.c_double * 9)(*M), m) else None


def _host_range(lib, m, size):
    return bool(lib.debig_png_persp_range((C.c_int64 * 9)(*m), size[1], size[0]))


def test_host_quantise_and_range_against_the_restatement(lib):
    rng = np.random.default_rng(30)
    seen = {True: 0, False: 0, None: 0}
    for k in range(3000):
        lin = rng.uniform(-1, 1, 4) * 10.0 ** rng.integers(-6, 5)
        tr = rng.uniform(-1, 1, 2) * 10.0 ** rng.integers(-3, 8)
        row2 = np.append(rng.uniform(-1, 1, 2) * 10.0 ** rng.integers(-6, 1), rng.uniform(0.2, 4.2))
        M = [lin[0], lin[1], tr[0], lin[2], lin[3], tr[1]] + [float(v) for v in row2]
        if k % 5 == 0:  # exact halves of a Q30 unit, both signs
            M[6 + k % 3] = (int(rng.integers(-1000, 1000)) + 0.5) / ONE
        want = PR.quantise(M)
        assert _host_q(lib, M) == want, M
        if want is None:
            seen[None] += 1
            continue
        size = (int(rng.integers(1, 300)), int(rng.integers(1, 300)))
        ok = PR.range_ok(want, size)
        seen[ok] += 1
        assert _host_range(lib, want, size) == ok, (want, size)
    assert min(seen.values()) > 100, seen
    for (cw, chh), size, M, m in _quads(10, 3):
        assert _host_q(lib, [v for r in M for v in r]) == m and _host_range(lib, m, size)
    for bad in (math.nan, math.inf, math.nextafter(4.0, 5.0), -math.nextafter(4.0, 5.0)):
        M = list(IDENT9)
        M[7] = bad
        assert _host_q(lib, M) is None
    assert _host_q(lib, [0] * 6 + [4.0, -4.0, 0.5 / ONE]) == [0] * 6 + [1 << 32, -(1 << 32), 1]


def test_host_range_at_the_limits(lib):
    """D exactly 2^21 and exactly 2^33 - 1 at a corner is accepted; one less or one more is refused"""
    W, H = 9, 5
    n = {True: 0, False: 0}
    for m, want, at, d in _corner_cases(W, H):
        assert _host_range(lib, m, (H, W)) == want, (m, at, d)
        n[want] += 1
    assert n[True] == 8 and n[False] >= 7, n
    ok = [0] * 6 + [0, 0, ONE]
    assert _host_range(lib, ok, (1, 1)) and _host_range(lib, ok, (16384, 16384))
    for size in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        assert not _host_range(lib, ok, size)
    for k in range(3):
        m = list(ok)
        m[6 + k] = (1 << 32) + 1 if k < 2 else -(1 << 32) - 1
        m[8] = m[8] if k == 2 else -(1 << 31)
        assert not _host_range(lib, m, (4, 4)) and not PR.range_ok(m, (4, 4))


# ---- the three C calls: what needs no device ------------------------------------------------------------------------------------------

def _persps(api, n, persps):
    if persps is None:
        return None
    ps = (api.PngPersp * n)()
    for i, m in enumerate([IDENT9] * n if persps == "ident" else persps):
        ps[i].m[:] = list(m)
    return ps


def _tensor_call(lib, api, files, desc, wd, out=DUMMY, boxes=None, persps="ident", colors=None, tones=None, tables=None, n_tables=0,
                 blurs=None):
    ins, sizes, st, bx, _ = TW._files(files, boxes, None)
    rc = lib.debig_png_decode_batch_tensor_persp(ins, sizes, out, bx, _persps(api, len(files), persps), colors, tones, tables, n_tables, blurs,
                                                 st, None, len(files), 0, C.byref(desc) if desc is not None else None,
                                                 C.byref(wd) if wd is not None else None)
    return rc, list(st)


def _label_call(lib, api, files, desc, wd, out=DUMMY, boxes=None, persps="ident"):
    ins, sizes, st, bx, _ = TW._files(files, boxes, None)
    rc = lib.debig_png_decode_batch_labels_persp(ins, sizes, out, bx, _persps(api, len(files), persps), st, None, len(files), 0,
                                                 C.byref(desc) if desc is not None else None, C.byref(wd) if wd is not None else None)
    return rc, list(st)


def _clbl_call(lib, api, files, desc, wd, out=DUMMY, boxes=None, persps="ident"):
    n = len(files)
    ins, sizes, st, bx, _ = TW._files(files, boxes, None)
    um = (C.c_uint32 * n)(*[SENTINEL] * n)
    rc = lib.debig_png_decode_batch_color_labels_persp(ins, sizes, out, bx, _persps(api, n, persps), st, None, um, n, 0,
                                                       C.byref(desc) if desc is not None else None, C.byref(wd) if wd is not None else None)
    return rc, list(st), list(um)


def test_tensor_argument_checks_leave_status_unwritten(lib, api):
    """every BAD_ARG path of the affine calls it stands for, before any file is read"""
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
        assert _tensor_call(lib, api, f, td(api), wd(api), persps=None, **extra) == (BAD_ARG, [SENTINEL])
        # neither the maps nor their descriptor: still refused, with tones or blurs as well (never a decode without a map)
        assert _tensor_call(lib, api, f, td(api), None, persps=None, **extra) == (BAD_ARG, [SENTINEL]), list(extra)
        assert _tensor_call(lib, api, f, td(api), wd(api), out=DUMMY + 8, **extra) == (BAD_ARG, [SENTINEL])
        assert _tensor_call(lib, api, f, td(api, fmt=4), wd(api), **extra) == (BAD_FORMAT, [SENTINEL])
    # the colour matrix needs RGB / RGBA; tone and blur need 8-bit samples and tables where they are counted
    assert _tensor_call(lib, api, f, td(api, fmt=TW.GRAY), wd(api), colors=cs) == (BAD_ARG, [SENTINEL])
    assert _tensor_call(lib, api, f, td(api, fmt=TW.GRAY), wd(api), colors=cs, tones=ts) == (BAD_ARG, [SENTINEL])
    for extra in (dict(tones=ts), dict(blurs=bs)):
        assert _tensor_call(lib, api, f, td(api, fmt=TW.RGB | TW.D16), wd(api, border=(0, 0, 0, 0)), **extra) == (BAD_ARG, [SENTINEL])
        assert _tensor_call(lib, api, f, td(api), wd(api), n_tables=1, **extra) == (BAD_ARG, [SENTINEL])
    assert lib.debig_png_decode_batch_tensor_persp(None, None, None, None, None, None, None, None, 0, None, None, None, 0, 0, None, None) == 0
    # at the edge of their ranges the arguments pass and the file is reached
    for desc, w in ((td(api), wd(api, filter=TW.NEAREST, border_mode=1)), (td(api), wd(api, border=(255, 255, 255, 256))),
                    (td(api, fmt=TW.RGBA | TW.D16, dtype=3), wd(api, border=(65535,) * 4)),
                    (td(api), wd(api, border_mode=1, border=(999, 999, 999, 999)))):
        assert _tensor_call(lib, api, f, desc, w) == (0, [R.E_SIGNATURE])
    for extra in (dict(colors=cs), dict(tones=ts), dict(blurs=bs), dict(colors=cs, tones=ts, blurs=bs)):
        assert _tensor_call(lib, api, f, td(api), wd(api), **extra) == (0, [R.E_SIGNATURE]), list(extra)


def test_label_argument_checks_leave_status_unwritten(lib, api):
    f = [b"not a png"]
    LD, LW = api.PngLabelDesc, api.PngLabelWarpDesc
    U8, U16, I32, I64 = range(4)
    bad = [(LD(out_w=8, out_h=6, dtype=U8), LW(0, 256)), (LD(out_w=8, out_h=6, dtype=U8), LW(0, -1)),
           (LD(out_w=8, out_h=6, dtype=U16), LW(0, 65536)), (LD(out_w=8, out_h=6, dtype=U16), LW(0, -1)),
           (LD(out_w=8, out_h=6, dtype=I64), LW(2, 0)), (LD(out_w=8, out_h=6, dtype=I64), None), (None, LW(0, 0)),
           (LD(out_w=0, out_h=6, dtype=I64), LW(0, 0)), (LD(out_w=8, out_h=6, dtype=4), LW(0, 0)),
           (LD(out_w=8, out_h=6, dtype=I32, reserved=1), LW(0, 0))]
    for desc, wd in bad:
        assert _label_call(lib, api, f, desc, wd) == (BAD_ARG, [SENTINEL]), (desc, wd)
    assert _label_call(lib, api, f, LD(out_w=8, out_h=6, dtype=I64), LW(0, 0), persps=None) == (BAD_ARG, [SENTINEL])
    assert lib.debig_png_decode_batch_labels_persp(None, None, None, None, None, None, None, 0, 0, None, None) == 0
    for desc, wd in ((LD(out_w=8, out_h=6, dtype=U8), LW(0, 255)), (LD(out_w=8, out_h=6, dtype=I32), LW(0, -1)),
                     (LD(out_w=8, out_h=6, dtype=U8), LW(1, -1))):
        assert _label_call(lib, api, f, desc, wd) == (0, [R.E_SIGNATURE])


def test_color_label_argument_checks_leave_status_and_unmatched_unwritten(lib, api):
    f = [b"not a png", b"x"]
    untouched = (BAD_ARG, [SENTINEL] * 2, [SENTINEL] * 2)
    LW = api.PngLabelWarpDesc
    one = [CC._map([1, 2, 3])]
    pack = CC._desc()
    u8 = CC._desc(dtype=0, mode=1, missing=0, maps=one)
    assert _clbl_call(lib, api, f, pack, LW(0, 0), persps=None) == untouched
    assert _clbl_call(lib, api, f, pack, None) == untouched
    assert _clbl_call(lib, api, f, pack, LW(2, 0)) == untouched
    for wd in (LW(0, 256), LW(0, -1)):
        assert _clbl_call(lib, api, f, u8, wd) == untouched
    cases = CC.bad_arg_cases(2)  # every inherited check, with valid and with missing perspective arguments
    assert len(cases) >= 30
    for name, desc, off in cases:
        out = None if off is None else DUMMY + off
        assert _clbl_call(lib, api, f, desc, LW(0, 0), out) == untouched, name
        assert _clbl_call(lib, api, f, desc, None, out, persps=None) == untouched, name
    assert _clbl_call(lib, api, f, u8, LW(1, 256)) == (0, [R.E_SIGNATURE] * 2, [0, 0])
    assert lib.debig_png_decode_batch_color_labels_persp(None, None, None, None, None, None, None, None, 0, 0, None, None) == 0


def test_warp_status_is_decided_on_the_host_behind_label_and_box(lib, api):
    """E_LABEL, then E_BOX, then E_WARP -- a non-finite entry, an entry beyond its limit, a horizon through the output, D below
    2^21 at one corner only --, each ahead of what the file holds later; a matrix that is fine on a small output is E_WARP on a
    larger one"""
    rng = np.random.default_rng(4)
    rgb = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    g8 = R.encode(R.random_image(rng, 9, 7, 0, 8), 0, 8)
    g8_crc = bytearray(g8)
    g8_crc[-20] ^= 1
    nan = (1, 0, 0, 0, 1, 0, 0, math.nan, 1)
    big = (1, 0, 0, 0, 1, 0, 4.5, 0, 1)
    affine_big = (1, 32768.5, 0, 0, 1, 0, 0, 0, 1)
    horizon = (1, 0, 0, 0, 1, 0, -0.25, 0, 1)        # D = 1 - 0.25 (X + 1/2): zero at X = 3.5, negative to the right of it
    near = (1, 0, 0, 0, 1, 0, 0, -1 / 5.5, 1.0)      # D = 0 at the centre of the last row's pixels (Y = 5)
    for M, size in ((horizon, (6, 8)), (near, (6, 8))):
        assert not PR.range_ok(PR.quantise(M), size) and PR.range_ok(PR.quantise(M), (3, 3))
    L, B, Wp = LR.E_LABEL, LR.E_BOX, WR.E_WARP
    # E_LABEL > E_BOX (file 0), E_LABEL > E_WARP (1), E_BOX > E_WARP (2), E_WARP > CRC (3), E_WARP > missing IDAT (4), E_WARP by
    # rows 0 and 1 (5); a walk error before the end of IHDR stands (6, 7)
    files = [rgb, rgb, g8, bytes(g8_crc), g8[:40], g8, g8[:30], b"\x89PNG"]
    boxes = [(0, 0, 10, 1), None, (0, 0, 10, 1), None, None, None, None, None]
    maps = [nan, nan, big, horizon, near, affine_big, big, nan]
    ld = api.PngLabelDesc(out_w=8, out_h=6, dtype=3)
    assert _label_call(lib, api, files, ld, api.PngLabelWarpDesc(0, -1), boxes=boxes, persps=maps) == \
        (0, [L, L, B, Wp, Wp, Wp, R.E_CHUNK, R.E_SIGNATURE])
    # the tensor call has no E_LABEL: the RGB files' box and matrix decide; the same with a blur per file
    for extra in (dict(), dict(blurs=(api.PngBlur * 8)()), dict(tones=(api.PngTone * 8)(), colors=(api.PngColor * 8)())):
        assert _tensor_call(lib, api, files, TW._tdesc(api), TW._wdesc(api), boxes=boxes, persps=maps, **extra) == \
            (0, [B, Wp, B, Wp, Wp, Wp, R.E_CHUNK, R.E_SIGNATURE]), list(extra)
    # the colour-label call: E_LABEL is a 16-bit file
    rgb16 = R.encode(R.random_image(rng, 9, 7, 2, 16), 2, 16)
    rc, st, um = _clbl_call(lib, api, [rgb16, rgb, rgb, rgb[:40]], CC._desc(), api.PngLabelWarpDesc(0, 0),
                            boxes=[None, (3, 3, 0, 2), None, None], persps=[nan, horizon, horizon, near])
    assert (rc, st, um) == (0, [CR.E_LABEL, CR.E_BOX, Wp, Wp], [0] * 4)


# ---- Python ------------------------------------------------------------------------------------------------------------------------------

def test_perspective_matrix_maps_the_four_points_onto_each_other(api):
    rng = np.random.default_rng(11)
    for k in range(30):
        src = rng.uniform(-20, 120, (4, 2)) if k else np.array([(0, 0), (50, 0), (50, 30), (0, 30.0)])
        dst = None if k % 2 else np.array([(0, 0), (64, 0), (64, 48), (0, 48.0)]) + rng.uniform(-5, 5, (4, 2))
        if k and not _convex(src):
            continue
        M = np.array(api.png_perspective_matrix(src, (48, 64), dst))
        assert M.shape == (3, 3) and M[2, 2] == 1.0
        for (x, y), (X, Y) in zip(src, dst if dst is not None else [(0, 0), (64, 0), (64, 48), (0, 48)]):
            u = M @ (X, Y, 1.0)
            assert np.allclose(u[:2] / u[2], (x, y), atol=1e-7), (k, u)
    # the crop's corners onto the output's corners at the crop's size: the identity
    assert np.allclose(api.png_perspective_matrix([(0, 0), (9, 0), (9, 5), (0, 5)], (5, 9)), np.eye(3), atol=1e-12)
    for bad in ([(0, 0), (1, 1), (2, 2), (3, 3)], [(0, 0)] * 4):
        with pytest.raises(ValueError):
            api.png_perspective_matrix(bad, (5, 9))
    with pytest.raises(ValueError):
        api.png_perspective_matrix([(0, 0), (1, 0), (1, 1)], (5, 9))
    assert api.png_perspective_from_warp(((0, -1, 5), (1, 0, 0.5))) == ((0, -1, 5), (1, 0, 0.5), (0, 0, 1))
    with pytest.raises(ValueError):
        api.png_perspective_from_warp(np.eye(3))


def _convex(q):
    e = [q[(i + 1) % 4] - q[i] for i in range(4)]
    s = [e[i][0] * e[(i + 1) % 4][1] - e[i][1] * e[(i + 1) % 4][0] for i in range(4)]
    return all(v > 1.0 for v in s) or all(v < -1.0 for v in s)


def test_python_keywords(api):
    import inspect

    sig = inspect.signature(api.png_decode_batch_tensor).parameters
    assert sig["perspective"].default is None and list(sig)[-1] == "filter"  # (`filter` stays the last parameter)
    for fn in (api.png_decode_batch_labels, api.png_decode_batch_color_labels):
        assert inspect.signature(fn).parameters["perspective"].default is None
    assert C.sizeof(api.PngPersp) == 72
    # perspective together with warp: refused, before any device is looked for
    for fn in (api.png_decode_batch_tensor, api.png_decode_batch_labels, api.png_decode_batch_color_labels):
        with pytest.raises(ValueError, match="exclude"):
            fn([b""], (4, 4), perspective=[None], warp=[None])
    # the rules of the warp descriptors hold under a perspective as well
    for kw in (dict(filter="bicubic"), dict(alpha="over"), dict(border="wrap"), dict(border="clamp", border_value=0.5)):
        with pytest.raises(ValueError):
            api.png_decode_batch_tensor([b""], (4, 4), perspective=[None], **kw)
    for fn in (api.png_decode_batch_labels, api.png_decode_batch_color_labels):
        for kw in (dict(border="mirror"), dict(border="clamp", border_label=3), dict(border_label=2 ** 31)):
            with pytest.raises(ValueError):
                fn([b""], (4, 4), perspective=[None], **kw)
    with pytest.raises(ValueError, match="one entry"):
        api._png_persps([None], 2)
    with pytest.raises(ValueError, match="3 x 3"):
        api._png_persps([((1, 0, 0), (0, 1, 0))], 1)
    ps = api._png_persps([None, np.arange(9).reshape(3, 3)], 2)
    assert list(ps[0].m) == list(IDENT9) and list(ps[1].m) == list(range(9))
    # without warp and perspective the border keywords are still refused
    with pytest.raises(ValueError, match="need warp"):
        api.png_decode_batch_tensor([b""], (4, 4), border="clamp")


def test_symbols_are_exported(lib):
    for name in ("debig_png_persp_quantise", "debig_png_persp_range", "debig_png_decode_batch_tensor_persp", "debig_png_decode_batch_labels_persp",
                 "debig_png_decode_batch_color_labels_persp", "debig_hip_png_persp_batch", "debig_hip_png_persp_color_batch",
                 "debig_hip_png_label_persp_batch", "debig_hip_png_color_label_persp_batch"):
        assert hasattr(lib, name), name


# ---- the sanitizer programs (stand-alone, plain child processes) ---------------------------------------------------------------------

@pytest.mark.parametrize("script", ["asan_png_persp.sh", "asan_png_persp_emu.sh"])
def test_stand_alone_programs_under_address_and_undefined_sanitizers(script, tmp_path):
    r = subprocess.run(["sh", os.path.join(ROOT, "tools", script), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
