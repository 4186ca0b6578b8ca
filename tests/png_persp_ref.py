"""TEST HELPER for the perspective warp (include/decode_png.h: debig_png_decode_batch_tensor_persp, _labels_persp,
_color_labels_persp): the rule in integers, on top of tests/png_warp_ref.py, and a float64 restatement for a sanity check.

  * quantise(M)                       -- nine Python integers (rows 0, 1: png_warp_ref.quantise; row 2: llround(M_2k 2^30)), or None;
  * range_ok(m, size)                 -- D in [2^21, 2^33 - 1] at the four corner pixels, |p_k| <= 2^32;
  * parts(size, m)                    -- NU, NV, D (H, W) int64 of every output pixel;
  * positions(size, m)                -- U, V (H, W) int64 (Q17) by the two-step division, every bound of the header asserted;
  * positions_wide(size, m)           -- the same as (N << 31) // D in Python integers (object arrays);
  * warp_int, warp, warp_labels, warp_color_labels, warp_mixed (the colour matrix)
                                      -- png_warp_ref / png_color_label_warp_ref / png_color_ref UNCHANGED, handed (U, V): their
                                         `positions` is replaced for the duration of the call, nothing behind it is restated here;
  * warp_float64(px, size, m, ..)     -- the bilinear map in float64 on the QUANTISED matrix, in sample units, and
  * float64_bound(P)                  -- how far the UINT result may lie from the rounded float64 one.

The float64 bound.  png_warp_ref's docstring derives d = 2^-14 M + 2^(P-17) samples (M = 2^P - 1) between the integer result
before its final shift and the exact bilinear value AT THE INTEGER POSITION (U, V).  Here the exact position is N 2^31 / D and
U is its floor: U / 2^17 lies at most 2^-17 pixels below it, on each axis.  The bilinear surface (border samples included) is
continuous and changes by at most |s01 - s00| <= M per pixel along an axis, also across a sample boundary, so the value at the
exact position differs from the one at (U, V) by at most 2 * 2^-17 * M samples.  Together
    d' = 2^-14 M + 2^(P-17) + 2^-16 M:   0.0175 + 0.0039 = 0.0214 at P = 8,   4.4999 + 1.0000 = 5.4999 at P = 16,
and with the two roundings to integers (1/2 each) and a float64 evaluation error far below 10^-6 (positions below 2^20 pixels
carry 2^-32 pixels of error; farther ones see only border or clamped samples) two integers within 1 + d' + 10^-6 differ by at
most floor(1 + d' + 10^-6): 1 at P = 8, 6 at P = 16.  It never reads the code under test."""
import contextlib
import math
from unittest import mock

import numpy as np

import png_warp_ref as WR

BILINEAR, NEAREST = WR.BILINEAR, WR.NEAREST
CONSTANT, CLAMP = WR.CONSTANT, WR.CLAMP
E_WARP = WR.E_WARP
D_MIN, D_MAX = 1 << 21, (1 << 33) - 1
_AFFINE_POSITIONS = WR.positions  # (the numerators; `positions` of that module is replaced while a warp of this one runs)


def quantise(M):
    M = [float(x) for x in np.asarray(M, dtype=np.float64).reshape(-1)]
    assert len(M) == 9
    out = WR.quantise(M[:6])
    if out is None:
        return None
    for x in M[6:]:
        if not math.isfinite(x) or abs(x) > 4.0:
            return None
        y = abs(x) * float(1 << 30)  # exact: a power of two
        n = math.floor(y)
        n += 1 if y - n >= 0.5 else 0
        out.append(-n if x < 0 else n)
    return out


def range_ok(m, size):
    H, W = size
    p = [int(v) for v in m[6:]]
    if not (1 <= W <= 16384 and 1 <= H <= 16384) or any(abs(v) > 1 << 32 for v in p):
        return False
    return all(D_MIN <= p[0] * cx + p[1] * cy + 2 * p[2] <= D_MAX for cx in (1, 2 * W - 1) for cy in (1, 2 * H - 1))


def parts(size, m):
    H, W = size
    m = [int(v) for v in m]
    NU, NV = _AFFINE_POSITIONS(size, m[:6])  # (asserts the limits of rows 0 and 1 and |N| < 2^48)
    assert all(abs(v) <= 1 << 32 for v in m[6:])
    cx = (2 * np.arange(W, dtype=np.int64) + 1)[None, :]
    cy = (2 * np.arange(H, dtype=np.int64) + 1)[:, None]
    D = m[6] * cx + m[7] * cy + 2 * m[8]  # |D| < 2^49
    return NU, NV, D


def positions(size, m):
    NU, NV, D = parts(size, m)
    assert D.min() >= D_MIN and D.max() <= D_MAX, "the map is out of range on this output (E_WARP)"
    assert range_ok(m, size)  # (the corners say the same: D is linear)
    out = []
    for N in (NU, NV):
        q1 = N // D  # numpy's // floors
        r1 = N - q1 * D
        assert r1.min() >= 0 and (r1 < D).all() and np.abs(q1).max() <= 1 << 27
        lo = (r1.astype(np.uint64) << np.uint64(31)) // D.astype(np.uint64)  # r1 << 31 < 2^64 because D < 2^33
        assert lo.max() < 1 << 31
        U = (q1 << 31) + lo.astype(np.int64)
        assert np.abs(U).max() < 1 << 59
        out.append(U)
    return out[0], out[1]


def positions_wide(size, m):
    NU, NV, D = parts(size, m)
    f = np.frompyfunc(lambda n, d: (int(n) << 31) // int(d), 2, 1)
    return f(NU, D), f(NV, D)


@contextlib.contextmanager
def _handing_over(m):
    with mock.patch.object(WR, "positions", lambda size, _m6: positions(size, m)):
        yield


def picks(size, m):
    U, V = positions(size, m)
    return U >> 17, V >> 17


def warp_int(px, size, m, *a, **kw):
    with _handing_over(m):
        return WR.warp_int(px, size, m[:6], *a, **kw)


def warp(px, size, m, *a, **kw):
    with _handing_over(m):
        return WR.warp(px, size, m[:6], *a, **kw)


def warp_labels(lab, size, m, *a, **kw):
    with _handing_over(m):
        return WR.warp_labels(lab, size, m[:6], *a, **kw)


def warp_color_labels(px, size, m, *a, **kw):
    import png_color_label_warp_ref as CW

    with _handing_over(m):
        return CW.warp_color_labels(px, size, m[:6], *a, **kw)


def warp_mixed(px, size, m, *a, **kw):
    """png_color_ref.warp (the colour matrix between the filter and the conversion) under the projective map"""
    import png_color_ref as CR

    with _handing_over(m):
        return CR.warp(px, size, m[:6], *a, **kw)


def warp_float64(px, size, m, mode=CONSTANT, border=(0, 0, 0, 0)):
    """the bilinear map in float64 on the quantised matrix, at the EXACT position N 2^31 / D -> (H, W, C) float64, not rounded"""
    NU, NV, D = parts(size, m)
    d = D.astype(np.float64)  # exact: |N| < 2^48, D < 2^33
    tu, tv = NU.astype(np.float64) / d * 16384.0 - 0.5, NV.astype(np.float64) / d * 16384.0 - 0.5  # U / 2^17 = N / D 2^14
    fx, fy = np.floor(tu), np.floor(tv)
    px_, py_ = (tu - fx)[:, :, None], (tv - fy)[:, :, None]
    ix, iy = np.clip(fx, -2.0 ** 40, 2.0 ** 40).astype(np.int64), np.clip(fy, -2.0 ** 40, 2.0 ** 40).astype(np.int64)
    t = [WR._tap(px, ix + dx, iy + dy, mode, border).astype(np.float64) for dy in (0, 1) for dx in (0, 1)]
    return (1.0 - py_) * ((1.0 - px_) * t[0] + px_ * t[1]) + py_ * ((1.0 - px_) * t[2] + px_ * t[3])


def float64_bound(P):
    """the largest |UINT result - floor(float64 result + 1/2)| the rule allows (the derivation is in the module docstring)"""
    M = (1 << P) - 1
    d = M / 16384.0 + 2.0 ** (P - 17) + 2.0 * M / 131072.0
    return math.floor(1.0 + d + 1e-6)

