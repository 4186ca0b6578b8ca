"""TEST HELPER for the affine warp (include/decode_png.h: debig_png_decode_batch_tensor_warp, debig_png_decode_batch_labels_warp):
the rule in integers, and a float64 restatement of the same map for a sanity check.

  * quantise(M)                   -- the six Python integers llround(M_k * 65536), or None on the E_WARP conditions;
  * positions(size, m)            -- U, V (H, W) int64 of every output pixel (Q17);
  * picks(size, m)                -- the nearest pick (jx, jy) = (U >> 17, V >> 17), unclamped;
  * warp_int(px, size, m, ...)    -- v (H, W, C) int64, the sample times 2^(30 - P), by the integer rule;
  * warp(px, size, m, ...)        -- the output elements (png_resize_ref.convert: the ONE conversion of the resize);
  * warp_labels(lab, size, m, ..) -- the label tensor of one image;
  * warp_float64(px, size, m, ..) -- the bilinear map in float64 on the QUANTISED matrix, in sample units, and
  * float64_bound(P)              -- how far the UINT result may lie from the rounded float64 one.

The float64 bound.  Write phi = f / 2^17 for the exact fraction of an axis, s in [0, M] (M = 2^P - 1) for the four taps (border
samples included) and e for the exact bilinear value.  Three steps of the integer rule round:
  1. w1 = (f + 4) >> 3 is f / 8 rounded half up, so |w1 / 16384 - phi| <= 2^-15 on each axis.  On the horizontal axis that moves
     a row's value by at most 2^-15 |s01 - s00| <= 2^-15 M;
  2. Hq = (h + 2^(P-3)) >> (P-2) is the row's value times 2^(16-P), rounded: at most half a unit, 2^(P-17) samples.  Hq / 2^(16-P)
     stays inside [0, M] (h <= 16384 M), so the two rows still differ by at most M;
  3. the vertical weights move the result by at most 2^-15 M again; the convex combination of the rows does not enlarge the
     errors of steps 1 and 2.
Before the final shift the integer result is therefore within d = 2^-14 M + 2^(P-17) samples of e: 0.0175 at P = 8, 4.4999 at
P = 16.  The UINT conversion rounds to the nearest integer (at most 1/2 more), the float64 restatement rounds e (at most 1/2),
and the float64 evaluation itself errs by far less than 10^-6: two integers that lie within 1 + d + 10^-6 of each other differ by
at most floor(1 + d + 10^-6) -- 1 at P = 8, 5 at P = 16."""
import math

import numpy as np

import png_resize_ref as Z

BILINEAR, NEAREST = 0, 2
CONSTANT, CLAMP = 0, 1
E_WARP = 16
LIN_MAX, TR_MAX = 32768.0, float(1 << 24)


def quantise(M):
    """M: six floats (row major) -> [m_k] Python integers, or None: a non-finite entry, a linear entry above 32768 or a
    translation above 2^24 in magnitude.  llround: halves go away from zero (the product by 65536 is exact in float64)."""
    M = [float(x) for x in np.asarray(M, dtype=np.float64).reshape(-1)]
    assert len(M) == 6
    out = []
    for k, x in enumerate(M):
        if not math.isfinite(x) or abs(x) > (TR_MAX if k in (2, 5) else LIN_MAX):
            return None
        y = abs(x) * 65536.0
        n = math.floor(y)
        n += 1 if y - n >= 0.5 else 0  # (y - floor(y) is exact)
        out.append(-n if x < 0 else n)
    return out


def positions(size, m):
    H, W = size
    cx = (2 * np.arange(W, dtype=np.int64) + 1)[None, :]
    cy = (2 * np.arange(H, dtype=np.int64) + 1)[:, None]
    m = [int(v) for v in m]
    assert all(abs(v) <= 1 << 31 for v in (m[0], m[1], m[3], m[4])) and abs(m[2]) <= 1 << 40 and abs(m[5]) <= 1 << 40
    U = m[0] * cx + m[1] * cy + 2 * m[2]
    V = m[3] * cx + m[4] * cy + 2 * m[5]
    assert np.abs(U).max() < 1 << 48 and np.abs(V).max() < 1 << 48
    return U, V


def picks(size, m):
    U, V = positions(size, m)
    return U >> 17, V >> 17


def _tap(px, jx, jy, mode, border):
    """px (h, w, C) -> samples (H, W, C) int64 at the (H, W) index arrays jx, jy; outside the crop: border (CONSTANT) or the
    clamped index (CLAMP)"""
    h, w, C = px.shape
    inside = (jx >= 0) & (jx < w) & (jy >= 0) & (jy < h)
    s = px[np.clip(jy, 0, h - 1), np.clip(jx, 0, w - 1)].astype(np.int64)
    if mode == CONSTANT:
        s[~inside] = np.asarray(border, np.int64)[:C]
    return s


def warp_int(px, size, m, filt=BILINEAR, mode=CONSTANT, border=(0, 0, 0, 0), box=None):
    """px: (h, w, C) uint8 / uint16 decoded pixels; box = (x, y, w, h) or None -> (v (H, W, C) int64, P)"""
    P = 8 * px.dtype.itemsize
    if box is not None and (box[2] or box[3]):
        x, y, w, h = box
        px = px[y:y + h, x:x + w]
    U, V = positions(size, m)
    if filt == NEAREST:
        return _tap(px, U >> 17, V >> 17, mode, border) << (30 - P), P
    tu, tv = U - 65536, V - 65536
    ix, iy = tu >> 17, tv >> 17
    w1x, w1y = (((tu & 0x1FFFF) + 4) >> 3)[:, :, None], (((tv & 0x1FFFF) + 4) >> 3)[:, :, None]
    w0x, w0y = Z.ONE - w1x, Z.ONE - w1y
    rnd, sh = 1 << (P - 3), P - 2
    h0 = (w0x * _tap(px, ix, iy, mode, border) + w1x * _tap(px, ix + 1, iy, mode, border) + rnd) >> sh
    h1 = (w0x * _tap(px, ix, iy + 1, mode, border) + w1x * _tap(px, ix + 1, iy + 1, mode, border) + rnd) >> sh
    assert h0.max() < 1 << 16 and h1.max() < 1 << 16
    v = w0y * h0 + w1y * h1
    assert v.max() < 1 << 30
    return v, P


def warp(px, size, m, filt=BILINEAR, dtype="uint", mode=CONSTANT, border=(0, 0, 0, 0), box=None, scale=(1, 1, 1, 1),
         bias=(0, 0, 0, 0), layout="hwc"):
    v, P = warp_int(px, size, m, filt, mode, border, box)
    out = Z.convert(v, P, dtype, scale, bias)
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1))) if layout == "chw" else out


def warp_labels(lab, size, m, mode=CONSTANT, border_label=0, box=None, lut=None, dtype="int64"):
    """lab (h, w) raw labels -> (H, W) of dtype; an outside pick under CONSTANT is border_label itself (not through the lut)"""
    import png_label_ref as LR

    if box is not None and (box[2] or box[3]):
        x, y, w, h = box
        lab = lab[y:y + h, x:x + w]
    h, w = lab.shape
    jx, jy = picks(size, m)
    inside = (jx >= 0) & (jx < w) & (jy >= 0) & (jy < h)
    v = lab[np.clip(jy, 0, h - 1), np.clip(jx, 0, w - 1)].astype(np.int64)
    if lut is not None:
        v = np.asarray(lut, dtype=np.int64)[v]
    if mode == CONSTANT:
        v[~inside] = border_label
    return v.astype(LR.DTYPES[dtype])


def warp_float64(px, size, m, mode=CONSTANT, border=(0, 0, 0, 0)):
    """the bilinear map in float64 on the quantised matrix -> (H, W, C) float64 in sample units (not rounded)"""
    U, V = positions(size, m)
    tu, tv = (U - 65536).astype(np.float64) / 131072.0, (V - 65536).astype(np.float64) / 131072.0  # exact: |U| < 2^48
    fx, fy = np.floor(tu), np.floor(tv)
    px_, py_ = (tu - fx)[:, :, None], (tv - fy)[:, :, None]
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    t = [_tap(px, ix + dx, iy + dy, mode, border).astype(np.float64) for dy in (0, 1) for dx in (0, 1)]
    return (1.0 - py_) * ((1.0 - px_) * t[0] + px_ * t[1]) + py_ * ((1.0 - px_) * t[2] + px_ * t[3])


def float64_bound(P):
    """the largest |UINT result - floor(float64 result + 1/2)| the rule allows (the derivation is in the module docstring)"""
    d = ((1 << P) - 1) / 16384.0 + 2.0 ** (P - 17)
    return math.floor(1.0 + d + 1e-6)
