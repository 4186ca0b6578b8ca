"""TEST TOOLING: numpy restatement of the filters of debig_png_decode_batch_tensor_filter (include/decode_png.h): the NEAREST
and BICUBIC weight rules in integers, the two SIGNED passes of the bicubic filter with their biased 16-bit intermediate and
their clamps, and the alpha modes on top of them.  The premultiply, the composite and the one final conversion are those of
png_alpha_ref / png_resize_ref, which this file imports; BILINEAR is png_resize_ref / png_alpha_ref unchanged.  Everything is
integer up to the conversion, so the kernel, the host, the emulator and this file agree bit for bit."""
import numpy as np

import png_alpha_ref as A
import png_resize_ref as Z

BILINEAR, BICUBIC, NEAREST = 0, 1, 2
FILTERS = {"bilinear": BILINEAR, "bicubic": BICUBIC, "nearest": NEAREST}
ONE = Z.ONE
MAX_SCALE_CUBIC = 32
MAX_ABS_SUM = 32768


def cubic_n(m, D):
    """the Keys kernel (a = -1/2) at the distance m / D filter units, times 2^29: u = m * 2^16 div D, two cubic pieces"""
    u = (m * 65536) // D
    if u <= 65536:
        p = 3 * u ** 3 - 327680 * u ** 2 + (1 << 49)
    else:
        p = -u ** 3 + 327680 * u ** 2 - (1 << 35) * u + (1 << 50)
    assert abs(p) < 1 << 55
    return p >> 20  # (Python's >> is arithmetic)


def taps(filt, cl, L, aa, X):
    """(first source index, [Q14 weights]) of output coordinate X, or None where the rule gives no table (T <= 0 or
    sum |w| > 32768); cl: crop length, L: output length"""
    filt = FILTERS.get(filt, filt)
    if filt == BILINEAR:
        return Z.taps(cl, L, aa, X)
    if filt == NEAREST:
        return ((2 * X + 1) * cl) // (2 * L), [ONE]
    assert filt == BICUBIC
    D = 2 * cl if aa and cl > L else 2 * L
    assert not (aa and cl > MAX_SCALE_CUBIC * L)
    c = (2 * X + 1) * cl
    js = [j for j in range(max((c - 2 * D) // (2 * L) - 1, 0), min((c + 2 * D) // (2 * L) + 2, cl)) if abs((2 * j + 1) * L - c) < 2 * D]
    assert js and js == list(range(js[0], js[0] + len(js)))
    assert (js[0] == 0 or abs((2 * js[0] - 1) * L - c) >= 2 * D) and (js[-1] == cl - 1 or abs((2 * js[-1] + 3) * L - c) >= 2 * D)
    ns = [cubic_n(abs((2 * j + 1) * L - c), D) for j in js]
    T = sum(ns)
    if T <= 0:
        return None
    w = [(n * ONE + (T >> 1)) // T for n in ns]  # (Python's // rounds toward minus infinity)
    w[ns.index(max(ns))] += ONE - sum(w)
    if sum(abs(x) for x in w) > MAX_ABS_SUM:
        return None
    return js[0], w


_AXES = {}


def axis(filt, cl, L, aa):
    key = (FILTERS.get(filt, filt), cl, L, bool(aa))
    if key not in _AXES:
        if len(_AXES) > 4096:
            _AXES.clear()
        _AXES[key] = [taps(filt, cl, L, aa, X) for X in range(L)]
    return _AXES[key]


def _crop(px, box):
    if box is not None and (box[2] or box[3]):
        x, y, w, h = box
        px = px[y:y + h, x:x + w]
    return px


def cubic_passes(s, P, size, aa):
    """s (h, w, C) int64 samples at precision P -> v (H, W, C) int64 BEFORE the clamp: the sample times 2^(29 - P), signed"""
    h, w, C = s.shape
    H, W = size
    hq = np.empty((h, W, C), np.int64)
    for X, (f, wt) in enumerate(axis(BICUBIC, w, W, aa)):
        acc = np.tensordot(s[:, f:f + len(wt), :], np.array(wt, np.int64), axes=([1], [0]))
        assert np.abs(acc).max() < 1 << 31
        hq[:, X, :] = np.clip(((acc + (1 << (P - 2))) >> (P - 1)) + 16384, 0, 65535)
    v = np.empty((H, W, C), np.int64)
    for Y, (f, wt) in enumerate(axis(BICUBIC, h, H, aa)):
        v[Y] = np.tensordot(np.array(wt, np.int64), hq[f:f + len(wt)], axes=([0], [0])) - (1 << 28)
    assert np.abs(v).max() < 1 << 31
    return v


def resize_int(px, size, filt, aa=True, box=None):
    """px: (h, w, C) uint8 / uint16 -> (v30 (H, W, C) int64, the sample times 2^(30 - P), inside [0, Vmax]; P)"""
    filt = FILTERS.get(filt, filt)
    if filt == BILINEAR:
        return Z.resize_int(px, size, aa, box)
    P = 8 * px.dtype.itemsize
    px = _crop(px, box)
    h, w, _ = px.shape
    H, W = size
    if filt == NEAREST:  # one weight of 16384: both passes are exact, v30 is the chosen sample << (30 - P)
        iy = [taps(NEAREST, h, H, aa, Y)[0] for Y in range(H)]
        ix = [taps(NEAREST, w, W, aa, X)[0] for X in range(W)]
        return px[iy][:, ix].astype(np.int64) << (30 - P), P
    M = (1 << P) - 1
    v = cubic_passes(px.astype(np.int64), P, size, aa)
    return np.clip(v, 0, M << (29 - P)) << 1, P


def resize_alpha_int(px, size, filt, mode, aa=True, box=None, background=None):
    """the alpha modes: px RGBA / GRAY_ALPHA (alpha last) -> (v30 or v', P)"""
    filt = FILTERS.get(filt, filt)
    mode = A.MODES.get(mode, mode)
    assert mode in (A.PREMULTIPLIED, A.OVER)
    if filt == BILINEAR:
        return A.resize_alpha_int(px, size, mode, aa, box, background)
    p = A.premultiply(_crop(px, box))
    v, P = resize_int(p, size, filt, aa, None)  # (every channel clamped to [0, Vmax]: alpha's clamp among them)
    v[:, :, :-1] = np.minimum(v[:, :, :-1], v[:, :, -1:])  # then every colour to [0, v30_alpha]
    if mode == A.OVER:
        v = A.over(v, P, background)
    return v, P


def resize(px, size, filt, dtype="uint", aa=True, box=None, scale=(1, 1, 1, 1), bias=(0, 0, 0, 0), layout="hwc", alpha=A.STRAIGHT,
           background=None):
    """the tensor of debig_png_decode_batch_tensor_filter for one image (alpha "straight": px has the tensor's channels; else
    px has them WITH alpha, as png_alpha_ref.resize_alpha)"""
    alpha = A.MODES.get(alpha, alpha)
    if alpha == A.STRAIGHT:
        v, P = resize_int(px, size, filt, aa, box)
    else:
        v, P = resize_alpha_int(px, size, filt, alpha, aa, box, background)
    out = Z.convert(v, P, dtype, scale, bias)
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1))) if layout == "chw" else out


def box_ok(filt, box, w, h, size, aa):
    """the E_BOX rule per filter: box None or (x, y, w, h)"""
    filt = FILTERS.get(filt, filt)
    if filt == BILINEAR:
        return Z.box_ok(box, w, h, size, aa)
    if box is None or (box[2] == 0 and box[3] == 0):
        box = (0, 0, w, h)
    x, y, bw, bh = box
    if bw == 0 or bh == 0 or x + bw > w or y + bh > h:
        return False
    return not (filt == BICUBIC and aa and (bw > MAX_SCALE_CUBIC * size[1] or bh > MAX_SCALE_CUBIC * size[0]))
