"""TEST TOOLING: numpy restatement of the resize arithmetic of debig_png_decode_batch_tensor (include/decode_png.h): the
Q14 integer weights of one axis, the two integer passes, and the final conversion to uint8 / uint16 / float32 / float16 /
bfloat16.  Everything is integer up to the conversion, so the kernel, the host and this file agree bit for bit."""
import numpy as np

T_UINT, T_F32, T_F16, T_BF16 = 0, 1, 2, 3
DTYPES = {"uint": T_UINT, "float32": T_F32, "float16": T_F16, "bfloat16": T_BF16}
ONE = 16384
MAX_SCALE = 64
E_BOX = 14


def taps(cl, L, aa, X):
    """(first source index, [Q14 weights]) of output coordinate X; cl: crop length, L: output length"""
    if not aa or cl <= L:
        num = min(max((2 * X + 1) * cl - L, 0), (cl - 1) * 2 * L)
        i0, r = divmod(num, 2 * L)
        if i0 == cl - 1:
            return i0, [ONE]
        w1 = (r * ONE + L) // (2 * L)
        return i0, [ONE - w1, w1]
    assert cl <= MAX_SCALE * L
    c = (2 * X + 1) * cl
    j0 = max((c - 2 * cl) // (2 * L) - 1, 0)
    js, ns = [], []
    for j in range(j0, cl):
        nj = 2 * cl - abs((2 * j + 1) * L - c)
        if nj > 0:
            js.append(j)
            ns.append(nj)
        elif js:
            break
    assert js == list(range(js[0], js[0] + len(js)))
    T = sum(ns)
    w = [(nj * ONE + T // 2) // T for nj in ns]
    w[ns.index(max(ns))] += ONE - sum(w)
    return js[0], w


def axis(cl, L, aa):
    return [taps(cl, L, aa, X) for X in range(L)]


def resize_int(px, size, aa=True, box=None):
    """px: (h, w, C) uint8 / uint16 decoded pixels -> v (H, W, C) int64, the sample times 2^(30 - P); size = (H, W);
    box = (x, y, w, h) or None"""
    P = 8 * px.dtype.itemsize
    if box is not None and (box[2] or box[3]):
        x, y, w, h = box
        px = px[y:y + h, x:x + w]
    h, w, C = px.shape
    H, W = size
    s = px.astype(np.int64)
    hq = np.empty((h, W, C), np.int64)
    for X, (f, wt) in enumerate(axis(w, W, aa)):
        acc = np.tensordot(s[:, f:f + len(wt), :], np.array(wt, np.int64), axes=([1], [0]))
        assert acc.max() < 1 << (P + 14)
        hq[:, X, :] = (acc + (1 << (P - 3))) >> (P - 2)
    assert hq.max() < 1 << 16
    v = np.empty((H, W, C), np.int64)
    for Y, (f, wt) in enumerate(axis(h, H, aa)):
        v[Y] = np.tensordot(np.array(wt, np.int64), hq[f:f + len(wt)], axes=([0], [0]))
    assert v.max() < 1 << 30
    return v, P


def bf16_bits(f32):
    """float32 array -> bfloat16 bit patterns (uint16), round to nearest even"""
    u = np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def affine(P, scale, bias):
    """A_c, B_c (float32) of the float conversion"""
    a = (np.asarray(scale, np.float64) / ((2 ** P - 1) * 2.0 ** (30 - P))).astype(np.float32)
    return a, np.asarray(bias, np.float32)


def convert(v, P, dtype, scale=(1, 1, 1, 1), bias=(0, 0, 0, 0)):
    """v (H, W, C) -> the output elements: uint8 / uint16, float32, float16, or bfloat16 BIT PATTERNS as uint16"""
    dtype = DTYPES.get(dtype, dtype)
    if dtype == T_UINT:
        return ((v + (1 << (29 - P))) >> (30 - P)).astype(np.uint8 if P == 8 else np.uint16)
    C = v.shape[2]
    a, b = affine(P, scale, bias)
    f = v.astype(np.float32)  # v < 2^30: exact in int64 -> float32 is one rounding to nearest even
    f = (f * a[:C]).astype(np.float32)
    f = (f + b[:C]).astype(np.float32)
    if dtype == T_F32:
        return f
    if dtype == T_F16:
        with np.errstate(over="ignore"):
            return f.astype(np.float16)
    return bf16_bits(f)


def resize(px, size, dtype="uint", aa=True, box=None, scale=(1, 1, 1, 1), bias=(0, 0, 0, 0), layout="hwc"):
    v, P = resize_int(px, size, aa, box)
    out = convert(v, P, dtype, scale, bias)
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1))) if layout == "chw" else out


def box_ok(box, w, h, size, aa):
    """the E_BOX rule: box None or (x, y, w, h)"""
    if box is None or (box[2] == 0 and box[3] == 0):
        box = (0, 0, w, h)
    x, y, bw, bh = box
    if bw == 0 or bh == 0 or x + bw > w or y + bh > h:
        return False
    return not (aa and (bw > MAX_SCALE * size[1] or bh > MAX_SCALE * size[0]))
