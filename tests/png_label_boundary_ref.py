"""TEST TOOLING: the boundary rule of include/decode_png.h (debig_png_label_boundary) restated in numpy, by shifted compares over the
footprint -- no tiles, no passes, no distances.

    reach(radius, shape)                -> [reach[0], ..., reach[radius]]: the half-width of the window at a row distance of d
    footprint(radius, shape)            -> bool (2r + 1, 2r + 1): F[r + dy, r + dx] = |dx| <= reach[|dy|]
    boundary(img, table)                -> bool (H, W): element (x, y) is True iff an element at (x + dx, y + dy), |dy| <= r,
                                           |dx| <= table[|dy|], INSIDE the image, differs from it (the window is clipped)
    apply(labels, radius, shape, mode, value, status=None) -> what the call writes for a (N, H, W) array: RING boundary ? value :
                                           the element, in the dtype of the input; EDGE uint8 1 / 0.  An image whose status is
                                           not 0: under RING the input, under EDGE zeros (what api.png_label_boundary returns).
An int16 array is the uint16 bits (which is how the label calls hand out uint16); elements are compared whole."""
import numpy as np

SHAPES = {"square": 0, "diamond": 1, "disk": 2}  # DEBIG_PNG_BOUNDARY_*
MODES = {"ring": 0, "edge": 1}
MAX_RADIUS = 16


def _isqrt(v):
    s = 0
    while (s + 1) * (s + 1) <= v:
        s += 1
    return s


def reach(radius, shape):
    if shape == "square":
        return [radius] * (radius + 1)
    if shape == "diamond":
        return [radius - d for d in range(radius + 1)]
    assert shape == "disk", shape
    return [_isqrt(radius * radius - d * d) for d in range(radius + 1)]


def footprint(radius, shape):
    table = reach(radius, shape)
    F = np.zeros((2 * radius + 1, 2 * radius + 1), bool)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            F[radius + dy, radius + dx] = abs(dx) <= table[abs(dy)]
    return F


def boundary(img, table):
    img = np.asarray(img)
    H, W = img.shape
    r = len(table) - 1
    out = np.zeros((H, W), bool)
    for dy in range(-r, r + 1):
        for dx in range(-table[abs(dy)], table[abs(dy)] + 1):
            if (dy == 0 and dx == 0) or abs(dy) >= H or abs(dx) >= W:
                continue
            # a[y, x] against a[y + dy, x + dx] wherever both lie in the image
            ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
            xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
            out[ys, xs] |= img[ys, xs] != img[yd, xd]
    return out


def apply_image(img, table, mode, value=255):
    b = boundary(img, table)
    if mode == "edge":
        return b.astype(np.uint8)
    out = img.copy()
    out[b] = np.array(value).astype(img.dtype) if img.dtype != np.int16 else np.array(value, np.uint16).view(np.int16)
    return out


def apply(labels, radius, shape, mode, value=255, status=None):
    labels = np.asarray(labels)
    table = reach(radius, shape)
    out = np.zeros(labels.shape, np.uint8) if mode == "edge" else labels.copy()
    for i in range(labels.shape[0]):
        if status is None or status[i] == 0:
            out[i] = apply_image(labels[i], table, mode, value)
    return out
