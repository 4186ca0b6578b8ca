"""TEST TOOLING: the distance rule of include/decode_png.h (debig_png_label_distance) restated in numpy by brute force -- for every
element a minimum over all its sites; no passes, no envelopes.

    d2(img, to=None)                    -> (int64 (H, W): D2, bool (H, W): NONE).  to=None: the sites of an element are the elements
                                           that differ from it (DIFFERS); an int: the elements equal to it (TO_VALUE)
    finish(d2, none, cap, out)          -> cap, NONE and the format: "squared" int32 (NONE without a cap: INT32_MAX), "root" float32,
                                           np.sqrt(float64).astype(float32) (NONE without a cap: +inf)
    apply_image(img, to, cap, out)      -> finish(d2(...))
    apply(labels, to, cap, out, status) -> what api.png_label_distance returns for a (N, H, W) array; an image whose status is not
                                           0 comes back as zeros
    row_g(img, to)                      -> uint16 (H, W): the g plane of the rows kernel (include/debig_hip.h): bits 0 .. 14 the
                                           distance along the row to the nearest site in the row (0x7fff: none), bit 15 "differs
                                           from the element above" (DIFFERS only)
    separable(img, to)                  -> d2() again by the separable form of DESIGN.md, in pure python (a statement of the form,
                                           not of the kernels: minima over whole runs, no envelope)
An int16 array is the uint16 bits (which is how the label calls hand out uint16); elements are compared whole."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
G_NONE, G_ABOVE = 0x7FFF, 0x8000
CHUNK = 1 << 22  # elements x sites of one numpy block


def _whole(img):
    img = np.asarray(img)
    return img.view(np.uint16) if img.dtype == np.int16 else img


def _min_over(ex, ey, sx, sy):
    """for every element (ex, ey): the minimum over the sites (sx, sy) of the squared distance"""
    out = np.empty(ex.size, np.int64)
    step = max(1, CHUNK // max(1, sx.size))
    for k in range(0, ex.size, step):
        dx = ex[k: k + step, None] - sx[None, :]
        dy = ey[k: k + step, None] - sy[None, :]
        out[k: k + step] = (dx * dx + dy * dy).min(axis=1)
    return out


def d2(img, to=None):
    img = _whole(img)
    H, W = img.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    out = np.zeros((H, W), np.int64)
    none = np.zeros((H, W), bool)
    if to is not None:
        site = np.zeros((H, W), bool) if not np.iinfo(img.dtype).min <= to <= np.iinfo(img.dtype).max else img == img.dtype.type(to)
        if not site.any():
            none[:] = True
        else:
            out[:] = _min_over(xx.ravel(), yy.ravel(), xx[site], yy[site]).reshape(H, W)
        return out, none
    for v in np.unique(img):
        mine = img == v
        if mine.all():
            none[:] = True
        else:
            out[mine] = _min_over(xx[mine], yy[mine], xx[~mine], yy[~mine])
    return out, none


def finish(dist2, none, cap=None, out="squared"):
    cap = cap or 0
    if cap:
        r = np.where(none, cap * cap, np.minimum(dist2, cap * cap))
    else:
        r = np.where(none, INT32_MAX, dist2)
    if out == "squared":
        return r.astype(np.int32)
    assert out == "root", out
    f = np.sqrt(r.astype(np.float64)).astype(np.float32)
    if not cap:
        f[none] = np.inf
    return f


def apply_image(img, to=None, cap=None, out="squared"):
    return finish(*d2(img, to), cap, out)


def apply(labels, to=None, cap=None, out="squared", status=None):
    labels = np.asarray(labels)
    res = np.zeros(labels.shape, np.int32 if out == "squared" else np.float32)
    for i in range(labels.shape[0]):
        if status is None or status[i] == 0:
            res[i] = apply_image(labels[i], to, cap, out)
    return res


def row_g(img, to=None):
    img = _whole(img)
    H, W = img.shape
    g = np.full((H, W), G_NONE, np.int64)
    xs = np.arange(W)
    for y in range(H):
        row = img[y]
        if to is not None:
            s = xs[row == to] if np.iinfo(img.dtype).min <= to <= np.iinfo(img.dtype).max else xs[:0]
            groups = [(xs, s)]
        else:
            groups = [(xs[row == v], xs[row != v]) for v in np.unique(row)]
        for e, s in groups:
            if s.size:  # the minimum over the row's sites of (x - x')^2 is a perfect square
                g[y, e] = np.rint(np.sqrt(_min_over(e, np.zeros(e.size, np.int64), s, np.zeros(s.size, np.int64)))).astype(np.int64)
    if to is None and H > 1:
        g[1:] |= np.where(img[1:] != img[:-1], G_ABOVE, 0)
    return g.astype(np.uint16)


def separable(img, to=None):
    """DESIGN.md, "the separable form": g along the rows, then per column a minimum of g(x, y')^2 + (y - y')^2 -- over the whole column
    under TO_VALUE, over the maximal same-valued run that contains y, plus the two virtual sites of row distance 0 just above and just
    below the run, under DIFFERS"""
    img = _whole(img)
    H, W = img.shape
    g = (row_g(img, to) & G_NONE).astype(np.int64)
    out = np.zeros((H, W), np.int64)
    none = np.zeros((H, W), bool)
    for x in range(W):
        for y in range(H):
            if to is None:
                a = b = y
                while a > 0 and img[a - 1, x] == img[y, x]:
                    a -= 1
                while b + 1 < H and img[b + 1, x] == img[y, x]:
                    b += 1
                cands = [(y - (a - 1)) ** 2] if a > 0 else []
                cands += [((b + 1) - y) ** 2] if b + 1 < H else []
            else:
                a, b, cands = 0, H - 1, []
            cands += [int(g[k, x]) ** 2 + (y - k) ** 2 for k in range(a, b + 1) if g[k, x] != G_NONE]
            if cands:
                out[y, x] = min(cands)
            else:
                none[y, x] = True
    return out, none
