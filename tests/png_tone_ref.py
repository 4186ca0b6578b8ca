"""TEST HELPER for the tone curves of the tensor decode (include/decode_png.h: debig_png_decode_batch_tensor_tone): the rule in
integers, on the 8-bit result of the first stage.

  * histogram(img8, cc)            -- img8 (H, W, C) uint8 -> (cc, 256) counts of the first cc (colour) channels over all pixels;
  * table(op, param, hist)         -- the 256-entry table of one channel (list of Python integers), or None on the E_TONE
                                      conditions; hist: 256 counts (ignored by the fixed operations); TABLE is the caller's bytes
                                      and is not handled here;
  * tables(op, param, img8, cc, user=None) -- (cc, 256) uint8: one table per colour channel (user: the caller's 256 bytes);
  * apply(img8, luts, dtype, ...)  -- the colour channels through their tables, alpha unchanged, then the ONE conversion of
                                      png_resize_ref.convert on v = entry << 22;
  * tone(img8, op, param, ...)     -- histogram, tables and apply of one image;
  * pillow_autocontrast_table(lo, hi) -- Pillow's ImageOps.autocontrast table (cutoff 0) as it evaluates it, in doubles.
"""
import numpy as np

import png_resize_ref as Z

NONE, AUTOCONTRAST, EQUALIZE, POSTERIZE, SOLARIZE, TABLE = 0, 1, 2, 3, 4, 5
OPS = {"autocontrast": AUTOCONTRAST, "equalize": EQUALIZE, "posterize": POSTERIZE, "solarize": SOLARIZE, "table": TABLE}
E_TONE = 18
IDENTITY = list(range(256))


def colour_channels(ch):
    return ch if ch & 1 else ch - 1


def histogram(img8, cc):
    img8 = np.asarray(img8)
    assert img8.dtype == np.uint8 and img8.ndim == 3
    return np.stack([np.bincount(img8[:, :, c].reshape(-1), minlength=256) for c in range(cc)]).astype(np.int64)


def param_ok(op, param, n_tables=0):
    if op in (NONE, AUTOCONTRAST, EQUALIZE):
        return param == 0
    if op == POSTERIZE:
        return 1 <= param <= 8
    if op == SOLARIZE:
        return param <= 256
    if op == TABLE:
        return param < n_tables
    return False


def table(op, param, hist=None):
    if op == TABLE or not param_ok(op, param):
        return None
    if op == NONE:
        return list(IDENTITY)
    if op == POSTERIZE:
        return [i & ~((1 << (8 - param)) - 1) & 255 for i in range(256)]
    if op == SOLARIZE:
        return [i if i < param else 255 - i for i in range(256)]
    h = [int(x) for x in hist]
    assert len(h) == 256
    nzi = [i for i in range(256) if h[i]]
    if op == AUTOCONTRAST:
        if not nzi or nzi[-1] <= nzi[0]:
            return list(IDENTITY)
        lo, hi = nzi[0], nzi[-1]
        return [0 if i < lo else min(255, max(0, ((i - lo) * 255) // (hi - lo))) for i in range(256)]
    if len(nzi) < 2:
        return list(IDENTITY)
    step = (sum(h) - h[nzi[-1]]) // 255
    if step == 0:
        return list(IDENTITY)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))
        n += h[i]
    return lut


def tables(op, param, img8, cc, user=None):
    if op == TABLE:
        return np.stack([np.asarray(user, np.uint8).reshape(256)] * cc)
    hs = histogram(img8, cc)
    return np.array([table(op, param, hs[c]) for c in range(cc)], np.uint8)


def apply(img8, luts, dtype="uint", scale=(1, 1, 1, 1), bias=(0, 0, 0, 0), layout="hwc"):
    img8 = np.asarray(img8)
    ch = img8.shape[2]
    cc = len(luts)
    assert cc == colour_channels(ch)
    m = img8.copy()
    for c in range(cc):
        m[:, :, c] = np.asarray(luts[c], np.uint8)[img8[:, :, c]]
    out = Z.convert(m.astype(np.int64) << 22, 8, dtype, scale, bias)
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1))) if layout == "chw" else out


def tone(img8, op, param, dtype="uint", scale=(1, 1, 1, 1), bias=(0, 0, 0, 0), layout="hwc", user=None):
    cc = colour_channels(img8.shape[2])
    return apply(img8, tables(op, param, img8, cc, user), dtype, scale, bias, layout)


def pillow_autocontrast_table(lo, hi):
    """ImageOps.autocontrast, cutoff 0, one channel whose lowest / highest non-empty bins are lo / hi"""
    if hi <= lo:
        return list(IDENTITY)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return [min(255, max(0, int(ix * scale + offset))) for ix in range(256)]
