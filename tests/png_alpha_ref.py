"""TEST TOOLING: numpy restatement of the alpha arithmetic of debig_png_decode_batch_tensor_alpha (include/decode_png.h):
premultiply at source precision, the two integer passes of png_resize_ref on the premultiplied samples, and the composite
over a background in the 30-bit domain.  Everything is integer up to the one conversion of png_resize_ref.convert, so the
kernel, the emulator and this file agree bit for bit."""
import numpy as np

import png_resize_ref as Z

STRAIGHT, PREMULTIPLIED, OVER = 0, 1, 2
MODES = {"straight": STRAIGHT, "premultiplied": PREMULTIPLIED, "over": OVER}


def premultiply(px):
    """px (h, w, C) uint8 / uint16 with alpha LAST (C = 2 or 4) -> the same shape and dtype:
    p_c = (s_c * alpha + (M >> 1)) div M for the colour channels, p_alpha = alpha"""
    assert px.shape[2] in (2, 4)
    P = 8 * px.dtype.itemsize
    M = (1 << P) - 1
    s = px.astype(np.int64)
    p = s.copy()
    p[:, :, :-1] = (s[:, :, :-1] * s[:, :, -1:] + (M >> 1)) // M
    assert (p[:, :, :-1] <= s[:, :, -1:]).all()
    return p.astype(px.dtype)


def over(v, P, background):
    """v (H, W, C) int64 premultiplied in the 30-bit domain, alpha last -> v' (H, W, C - 1):
    v'_c = v_c + (b_c * (Vmax - v_alpha) + (M >> 1)) div M; background: C - 1 integers in 0 .. M"""
    M = (1 << P) - 1
    vmax = M << (30 - P)
    b = np.asarray(background, np.int64)[: v.shape[2] - 1]
    assert b.shape == (v.shape[2] - 1,) and (b >= 0).all() and (b <= M).all()
    t = vmax - v[:, :, -1:]
    assert (t >= 0).all()
    out = v[:, :, :-1] + (b * t + (M >> 1)) // M
    assert (out <= vmax).all()
    return out


def resize_alpha_int(px, size, mode, aa=True, box=None, background=None):
    """-> (v or v', P): the 30-bit values before the conversion"""
    mode = MODES.get(mode, mode)
    assert mode in (PREMULTIPLIED, OVER)
    if box is not None and (box[2] or box[3]):  # (premultiplying the crop only: the same values, less work)
        x, y, w, h = box
        px = px[y:y + h, x:x + w]
    v, P = Z.resize_int(premultiply(px), size, aa, None)
    assert (v[:, :, :-1] <= v[:, :, -1:]).all()
    if mode == OVER:
        v = over(v, P, background)
    return v, P


def resize_alpha(px, size, mode, dtype="uint", aa=True, box=None, background=None, scale=(1, 1, 1, 1), bias=(0, 0, 0, 0),
                 layout="hwc"):
    """px: RGBA or GRAY_ALPHA pixels (h, w, 4 | 2) -> the tensor of debig_png_decode_batch_tensor_alpha for one image:
    mode "premultiplied": all channels; "over": the colour channels composited over `background` (integers 0 .. 2^P - 1
    per output channel).  scale / bias are indexed by output channel."""
    v, P = resize_alpha_int(px, size, mode, aa, box, background)
    out = Z.convert(v, P, dtype, scale, bias)
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1))) if layout == "chw" else out


def background_samples(background, channels, P):
    """per-channel background on the [0, 1] scale (None: white; a number: every channel) -> integers round(x * M)"""
    M = (1 << P) - 1
    if background is None:
        background = 1.0
    b = [float(x) for x in (background if hasattr(background, "__len__") else [background] * channels)]
    assert len(b) == channels and all(0.0 <= x <= 1.0 for x in b)
    return [int(round(x * M)) for x in b]
