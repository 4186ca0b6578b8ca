"""TEST TOOLING: the component rule of include/decode_png.h (debig_png_label_components) restated in numpy as a FIXPOINT OF MINIMA --
every element starts with its own index y * W + x; a sweep gives both elements of every pair of neighbours the smaller of their two
labels and then replaces every label by the label of the element it names; sweeps repeat until nothing changes.  At the fixpoint
neighbours agree, so a label is constant on a component, and a label names an element that names itself, which can only be the
component's smallest element.  No trees, no unions, no atomics, no runs of rows.

    first(img, connectivity=4, background=None)  -> int32 (H, W): the FIRST of every element's component, background -1
    consecutive(first)                           -> (int32 (H, W): 1 .. K in increasing order of FIRST, background 0; K)
    apply(batch, connectivity, background, ids, status) -> what api.png_label_components returns for a (N, H, W) array: (int32
                                                    (N, H, W), int64 (N,) of K); an image whose status is not 0 comes back as zeros, K 0
An int16 array is the uint16 bits (which is how the label calls hand out uint16); elements are compared whole; a background that
the dtype cannot hold matches nothing."""
import numpy as np


def _whole(img):
    img = np.asarray(img)
    return img.view(np.uint16) if img.dtype == np.int16 else img


def background_mask(img, background):
    img = _whole(img)
    if background is None or not np.iinfo(img.dtype).min <= background <= np.iinfo(img.dtype).max:
        return np.zeros(img.shape, bool)
    return img == img.dtype.type(background)


def first(img, connectivity=4, background=None):
    assert connectivity in (4, 8)
    img = _whole(img)
    H, W = img.shape
    back = background_mask(img, background)
    lab = np.arange(H * W, dtype=np.int64).reshape(H, W)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    pairs = []  # (the view of the upper / left element, the view of the other one, whether they are neighbours)
    for dy, dx in steps:
        a = (slice(0, H - dy), slice(max(0, -dx), W - max(0, dx)))
        b = (slice(dy, H), slice(max(0, dx), W - max(0, -dx)))
        pairs.append((a, b, (img[a] == img[b]) & ~back[a]))
    flat = lab.reshape(-1)
    while True:
        old = lab.copy()
        for a, b, same in pairs:
            m = np.minimum(lab[a], lab[b])
            lab[a] = np.where(same, m, lab[a])
            lab[b] = np.where(same, np.minimum(m, lab[b]), lab[b])  # (the two views overlap: a label only ever gets smaller)
        flat[:] = flat[flat]
        if np.array_equal(lab, old):
            break
    return np.where(back, -1, lab).astype(np.int32)


def consecutive(fst):
    firsts = np.unique(fst[fst >= 0])
    out = np.where(fst >= 0, np.searchsorted(firsts, fst) + 1, 0).astype(np.int32)
    return out, int(firsts.size)


def apply(batch, connectivity=4, background=None, ids="consecutive", status=None):
    batch = _whole(batch)
    out = np.zeros(batch.shape, np.int32)
    counts = np.zeros(batch.shape[0], np.int64)
    for i, img in enumerate(batch):
        if status is not None and status[i] != 0:
            continue
        f = first(img, connectivity, background)
        c, counts[i] = consecutive(f)
        out[i] = f if ids == "first" else c
    return out, counts
