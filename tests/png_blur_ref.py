"""TEST HELPER for the Gaussian blur and the sharpness of the tensor decode (include/decode_png.h:
debig_png_decode_batch_tensor_blur): the rule in integers, on the 8-bit result of the stages in front.

  * param_ok(op, ksize, value)      -- the E_BLUR rule;
  * weights(ksize, sigma)           -- the ksize Q14 taps (Python integers) from the integer rule, or None for bad parameters;
                                       weights_real(ksize, sigma): the normalised double weights they quantise;
  * fold(i, n)                      -- index i of an axis of n samples, mirrored without repeating the edge (numpy array in, out);
  * gaussian_int(img8, ksize, sigma) -- img8 (H, W, C) uint8 -> v (H, W, C) int64, the sample in Q22, every channel;
  * smooth(img8)                    -- Pillow's ImageFilter.SMOOTH of every channel, uint8;
  * sharpness_int(img8, factor)     -- v in Q22: the colour channels blended with their SMOOTH, alpha (the last of 2 or 4) as it is;
  * blur(img8, op, ksize, value, dtype, ...) -- v through the ONE conversion of png_resize_ref.convert.
"""
import math

import numpy as np

import png_resize_ref as Z

NONE, GAUSSIAN, SHARPNESS = 0, 1, 2
OPS = {"gaussian": GAUSSIAN, "sharpness": SHARPNESS}
E_BLUR = 19
ONE = 16384


def colour_channels(ch):
    return ch if ch & 1 else ch - 1


def param_ok(op, ksize, value):
    if op == NONE:
        return True
    if op == GAUSSIAN:
        return ksize % 2 == 1 and 3 <= ksize <= 63 and math.isfinite(value) and 0 < value <= 1000
    if op == SHARPNESS:
        return math.isfinite(value) and abs(value) <= 16
    return False


def weights_real(ksize, sigma):
    r = ksize // 2
    w = np.exp(-0.5 * (np.arange(-r, r + 1, dtype=np.float64) / float(sigma)) ** 2)
    return w / w.sum()


def weights(ksize, sigma):
    if not param_ok(GAUSSIAN, ksize, sigma):
        return None
    q = [int(math.floor(float(x) * ONE + 0.5)) for x in weights_real(ksize, sigma)]
    q[ksize // 2] += ONE - sum(q)
    return q


def fold(i, n):
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def gaussian_int(img8, ksize, sigma):
    img8 = np.asarray(img8)
    assert img8.dtype == np.uint8 and img8.ndim == 3
    q = weights(ksize, sigma)
    H, W, _ = img8.shape
    r = ksize // 2
    p = img8.astype(np.int64)
    h = np.zeros_like(p)
    xs = np.arange(W)
    for j in range(-r, r + 1):
        h += q[j + r] * p[:, fold(xs + j, W), :]
    h16 = (h + 32) >> 6
    assert h16.max() <= 65280
    v = np.zeros_like(p)
    ys = np.arange(H)
    for j in range(-r, r + 1):
        v += q[j + r] * h16[fold(ys + j, H), :, :]
    assert v.max() <= 255 << 22
    return v


def smooth(img8):
    img8 = np.asarray(img8)
    assert img8.dtype == np.uint8 and img8.ndim == 3
    H, W, _ = img8.shape
    s = img8.copy()
    if H < 3 or W < 3:
        return s
    p = img8.astype(np.int64)
    acc = 4 * p[1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            acc = acc + p[dy:H - 2 + dy, dx:W - 2 + dx]
    s[1:-1, 1:-1] = ((2 * acc + 13) // 26).astype(np.uint8)
    return s


def sharpness_k(factor):
    return int(math.floor(abs(factor) * 65536 + 0.5)) * (1 if factor >= 0 else -1)  # llround: half away from zero


def sharpness_int(img8, factor):
    img8 = np.asarray(img8)
    cc = colour_channels(img8.shape[2])
    p = img8.astype(np.int64)
    s = smooth(img8).astype(np.int64)
    K = sharpness_k(factor)
    v = np.clip((s << 22) + K * (p - s) * 64, 0, 255 << 22)
    v[:, :, cc:] = p[:, :, cc:] << 22
    return v


def blur_int(img8, op, ksize, value):
    assert op in (GAUSSIAN, SHARPNESS) and param_ok(op, ksize, value)
    return gaussian_int(img8, ksize, value) if op == GAUSSIAN else sharpness_int(img8, value)


def blur(img8, op, ksize, value, dtype="uint", scale=(1, 1, 1, 1), bias=(0, 0, 0, 0), layout="hwc"):
    out = Z.convert(blur_int(img8, op, ksize, value), 8, dtype, scale, bias)
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1))) if layout == "chw" else out
