"""TEST HELPER for the elastic deformation (include/decode_png.h: debig_png_decode_batch_tensor_elastic, _labels_elastic,
_color_labels_elastic): the rule in integers, on top of tests/png_warp_ref.py, and a float64 restatement for a sanity check.

  * quantise_field(F)                 -- (gh, gw, 2) int64 llround(v 65536), or None on the E_WARP conditions;
  * cell(X, W, g)                     -- k, t of every coordinate of an axis (arrays);
  * weights(t)                        -- the four Q14 weights (4, ...) int64 of the fractions t;
  * displacement(size, q)             -- Dx, Dy (H, W) int64 (Q16) of every output pixel; q None: zeros;
  * positions(size, m, q)             -- U, V (H, W) int64 (Q17);
  * warp_int, warp, warp_labels, warp_color_labels, warp_mixed (the colour matrix)
                                      -- png_warp_ref / png_color_label_warp_ref / png_color_ref UNCHANGED, handed (U, V): their
                                         `positions` is replaced for the duration of the call, nothing behind it is restated here;
  * catmull_rom_float64(size, F)      -- the displacement in float64 from the UNQUANTISED field, exact node positions.
It never reads the code under test."""
import contextlib
import math
from unittest import mock

import numpy as np

import png_warp_ref as WR

BILINEAR, NEAREST = WR.BILINEAR, WR.NEAREST
CONSTANT, CLAMP = WR.CONSTANT, WR.CLAMP
E_WARP = WR.E_WARP
NODE_MAX = 1 << 28
ONE = 16384
_AFFINE_POSITIONS = WR.positions


def quantise_field(F):
    F = np.asarray(F, dtype=np.float64)
    assert F.ndim == 3 and F.shape[2] == 2
    if not np.isfinite(F).all() or (np.abs(F) > 4096.0).any():
        return None
    y = np.abs(F) * 65536.0  # exact: a power of two
    n = np.floor(y)
    n = n + (y - n >= 0.5)
    return (np.sign(F) * n).astype(np.int64)


def cell(X, W, g):
    X = np.asarray(X, dtype=np.int64)
    num, den = (2 * X + 1) * (g - 1), 2 * W
    k = num // den
    assert (k <= g - 2).all() and (k >= 0).all()
    t = ((num - k * den) * ONE + W) // den
    assert (t >= 0).all() and (t <= ONE).all()
    return k, t


def weights(t):
    t = np.asarray(t, dtype=np.int64)
    t2, t3 = t * t, t * t * t
    n = [-t3 + 2 * t2 * ONE - t * (1 << 28), 3 * t3 - 5 * t2 * ONE + 2 * (1 << 42), -3 * t3 + 4 * t2 * ONE + t * (1 << 28),
         t3 - t2 * ONE]
    w = [(v + (1 << 28)) >> 29 for v in n]  # numpy's >> on int64 is arithmetic
    low = t < 8192
    w1 = np.where(low, ONE - (w[0] + w[2] + w[3]), w[1])
    w2 = np.where(low, w[2], ONE - (w[0] + w[1] + w[3]))
    return np.stack([w[0], w1, w2, w[3]])


def displacement(size, q):
    H, W = size
    if q is None:
        return np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    q = np.asarray(q, dtype=np.int64)
    gh, gw = q.shape[:2]
    assert 2 <= gh <= 33 and 2 <= gw <= 33 and np.abs(q).max() <= NODE_MAX
    kx, tx = cell(np.arange(W), W, gw)
    ky, ty = cell(np.arange(H), H, gh)
    wx, wy = weights(tx), weights(ty)  # (4, W), (4, H)
    S = np.zeros((H, W, 2), dtype=np.int64)
    for i in range(4):
        ry = np.clip(ky - 1 + i, 0, gh - 1)
        for j in range(4):
            cx = np.clip(kx - 1 + j, 0, gw - 1)
            S += (wy[i][:, None] * wx[j][None, :])[:, :, None] * q[ry[:, None], cx[None, :]]
    assert np.abs(S).max() < 1 << 57
    D = (S + (1 << 27)) >> 28
    return D[:, :, 0], D[:, :, 1]


def positions(size, m, q):
    m = [int(v) for v in m]
    NU, NV = _AFFINE_POSITIONS(size, m)
    Dx, Dy = displacement(size, q)
    U = NU + ((m[0] * Dx + m[1] * Dy + (1 << 14)) >> 15)
    V = NV + ((m[3] * Dx + m[4] * Dy + (1 << 14)) >> 15)
    return U, V


@contextlib.contextmanager
def _handing_over(m, q):
    with mock.patch.object(WR, "positions", lambda size, _m6: positions(size, m, q)):
        yield


def picks(size, m, q):
    U, V = positions(size, m, q)
    return U >> 17, V >> 17


def warp_int(px, size, m, q, *a, **kw):
    with _handing_over(m, q):
        return WR.warp_int(px, size, m, *a, **kw)


def warp(px, size, m, q, *a, **kw):
    with _handing_over(m, q):
        return WR.warp(px, size, m, *a, **kw)


def warp_labels(lab, size, m, q, *a, **kw):
    with _handing_over(m, q):
        return WR.warp_labels(lab, size, m, *a, **kw)


def warp_color_labels(px, size, m, q, *a, **kw):
    import png_color_label_warp_ref as CW

    with _handing_over(m, q):
        return CW.warp_color_labels(px, size, m, *a, **kw)


def warp_mixed(px, size, m, q, *a, **kw):
    """png_color_ref.warp (the colour matrix between the filter and the conversion) under the elastic map"""
    import png_color_ref as CR

    with _handing_over(m, q):
        return CR.warp(px, size, m, *a, **kw)


def catmull_rom_float64(size, F):
    """the Catmull-Rom interpolation of the float64 field F (gh, gw, 2) at every output pixel centre, edge nodes replicated,
    exact cell and fraction -> (H, W, 2) float64 in output pixels"""
    H, W = size
    F = np.asarray(F, dtype=np.float64)
    gh, gw = F.shape[:2]

    def axis(n, N, g):
        p = (np.arange(n) + 0.5) * (g - 1) / N
        k = np.minimum(np.floor(p), g - 2).astype(np.int64)
        t = p - k
        w = np.stack([(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2,
                      (t ** 3 - t ** 2) / 2])
        return k, w

    kx, wx = axis(W, W, gw)
    ky, wy = axis(H, H, gh)
    out = np.zeros((H, W, 2))
    for i in range(4):
        ry = np.clip(ky - 1 + i, 0, gh - 1)
        for j in range(4):
            cx = np.clip(kx - 1 + j, 0, gw - 1)
            out += (wy[i][:, None] * wx[j][None, :])[:, :, None] * F[ry[:, None], cx[None, :]]
    return out


def weights_float64(t):
    """the real Keys polynomial (a = -1/2) at t / 16384, in units of 2^-14"""
    x = np.asarray(t, dtype=np.float64) / ONE
    return ONE * np.stack([(-x ** 3 + 2 * x ** 2 - x) / 2, (3 * x ** 3 - 5 * x ** 2 + 2) / 2, (-3 * x ** 3 + 4 * x ** 2 + x) / 2,
                           (x ** 3 - x ** 2) / 2])
