"""TEST HELPER for the per-image colour matrix (include/decode_png.h: debig_png_decode_batch_tensor_color,
debig_png_decode_batch_tensor_warp_color): the rule in integers, composed with the resize and the warp restatements.

  * quantise(M, P)                 -- (k [9 Python integers], o [3]) = (llround(m_cj * 65536), llround(m_c3 * Vmax)), or None on
                                      the E_COLOR conditions (a non-finite entry, |m| > 16);
  * mix(v, P, k, o)                -- v (H, W, C) int64, the sample times 2^(30 - P) -> the same with its first three channels
                                      mixed: clamp(((k . v + 32768) >> 16) + o, 0, Vmax); a fourth channel passes through;
  * resize(px, size, M, ...)       -- png_resize_ref / png_filter_ref's filter passes, the mix, the ONE conversion;
  * warp(px, size, m, M, ...)      -- png_warp_ref.warp_int, the mix, the ONE conversion;
  * mix_float64(x, M)              -- clip(M[:, :3] x + M[:, 3], 0, 1) in float64 on samples in [0, 1], and
  * float64_bound()                -- how far the UINT8 result of one pixel may lie from the rounded float64 one (levels).

The float64 bound, for P = 8 and |m| <= 2.  x_j = s_j / 255 exactly corresponds to v_j = s_j << 22 = x_j Vmax.  Three steps round:
  1. k_cj = llround(m_cj 2^16) is off by at most 2^-17 per coefficient: acc / 2^16 differs from sum m_cj v_j by at most
     3 * 2^-17 Vmax, that is 3 * 2^-17 * 255 = 0.0059 levels;
  2. (acc + 32768) >> 16 rounds to a unit of v: half a unit, 2^-23 levels; o_c = llround(m_c3 Vmax) likewise (and the float64
     product's own rounding is smaller still);
  3. the clamp is monotone and 1-Lipschitz, so it does not enlarge the difference; the UINT conversion rounds to the nearest level
     (1/2), as does the float64 restatement's own rounding of 255 * clip(...) (1/2).
Two integers that lie within 1 + 0.006 + 2^-22 of each other differ by at most 1 level."""
import math

import numpy as np

import png_resize_ref as Z
import png_warp_ref as WR

E_COLOR = 17
M_MAX = 16.0
IDENTITY = ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0))
NEGATIVE = ((-1.0, 0.0, 0.0, 1.0), (0.0, -1.0, 0.0, 1.0), (0.0, 0.0, -1.0, 1.0))


def vmax(P):
    return ((1 << P) - 1) << (30 - P)


def _llround(y):
    """halves away from zero; y - floor(y) is exact for |y| < 2^52"""
    a = abs(y)
    n = math.floor(a)
    n += 1 if a - n >= 0.5 else 0
    return -n if y < 0 else n


def quantise(M, P):
    M = [float(x) for x in np.asarray(M, dtype=np.float64).reshape(-1)]
    assert len(M) == 12 and P in (8, 16)
    if any(not math.isfinite(x) or abs(x) > M_MAX for x in M):
        return None
    k = [_llround(M[4 * c + j] * 65536.0) for c in range(3) for j in range(3)]
    o = [_llround(M[4 * c + 3] * float(vmax(P))) for c in range(3)]  # (the product as float64 rounds it)
    return k, o


def mix(v, P, k, o):
    v = np.asarray(v, np.int64)
    assert v.shape[2] in (3, 4) and v.min() >= 0 and v.max() < 1 << 30
    out = v.copy()
    for c in range(3):
        acc = int(k[3 * c]) * v[:, :, 0] + int(k[3 * c + 1]) * v[:, :, 1] + int(k[3 * c + 2]) * v[:, :, 2]
        assert np.abs(acc).max() < 1 << 52
        out[:, :, c] = np.clip(((acc + 32768) >> 16) + int(o[c]), 0, vmax(P))
    return out


def _finish(v, P, dtype, scale, bias, layout):
    out = Z.convert(v, P, dtype, scale, bias)
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1))) if layout == "chw" else out


def resize(px, size, M, filt="bilinear", dtype="uint", aa=True, box=None, scale=(1, 1, 1, 1), bias=(0, 0, 0, 0), layout="hwc"):
    """px (h, w, 3 or 4) uint8 / uint16 -> the tensor of one image; filt "bilinear" | "nearest"; M None: no mix"""
    if filt == "nearest":
        import png_filter_ref as FR

        v, P = FR.resize_int(px, size, FR.NEAREST, aa, box)
    else:
        v, P = Z.resize_int(px, size, aa, box)
    if M is not None:
        v = mix(v, P, *quantise(M, P))
    return _finish(v, P, dtype, scale, bias, layout)


def warp(px, size, m, M, filt=WR.BILINEAR, dtype="uint", mode=WR.CONSTANT, border=(0, 0, 0, 0), box=None, scale=(1, 1, 1, 1),
         bias=(0, 0, 0, 0), layout="hwc"):
    v, P = WR.warp_int(px, size, m, filt, mode, border, box)
    if M is not None:
        v = mix(v, P, *quantise(M, P))
    return _finish(v, P, dtype, scale, bias, layout)


def mix_float64(x, M):
    """x (..., 3) float64 in [0, 1] -> clip(M[:, :3] x + M[:, 3], 0, 1)"""
    M = np.asarray(M, np.float64).reshape(3, 4)
    return np.clip(x @ M[:, :3].T + M[:, 3], 0.0, 1.0)


def float64_bound():
    return math.floor(1.0 + 3 * 2.0 ** -17 * 255 + 2.0 ** -22)
