"""TEST TOOLING: the numpy restatement of the label statistics (include/decode_png.h: debig_png_label_stats has the rule).

    stats(labels, n_ids, status=None) -> int64 (N, n_ids + 1, 5): the PUBLIC records (count, x0, y0, x1, y1)
    to_raw(public, out_w, out_h) / to_public(raw, out_w, out_h): the RAW records of include/debig_hip.h (debig_png_label_stat:
    count, x_end = max x + 1, y_end = max y + 1, x_rev = out_w - min x, y_rev = out_h - min y; all zeros when the id is absent)

Written from the rule alone, one masked reduction per record: nothing of the kernel's order or tables is in it."""
import numpy as np


def key_of(labels, n_ids):
    """the record every element goes to: its value where that is in 0 .. n_ids - 1, else n_ids ("other").  uint16 handed out as
    int16 bits is read as uint16; int64 is compared whole"""
    a = np.asarray(labels)
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    assert a.dtype in (np.uint8, np.uint16, np.int32, np.int64), a.dtype
    a = a.astype(np.int64)
    return np.where((a >= 0) & (a < n_ids), a, n_ids)


def stats_image(img, n_ids):
    H, W = img.shape
    key = key_of(img, n_ids)
    out = np.zeros((n_ids + 1, 5), np.int64)
    for k in np.unique(key):
        ys, xs = np.nonzero(key == k)
        out[k] = (len(ys), xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return out


def stats(labels, n_ids, status=None):
    labels = np.asarray(labels)
    assert labels.ndim == 3 and 1 <= n_ids <= 1024
    out = np.zeros((labels.shape[0], n_ids + 1, 5), np.int64)
    for i in range(labels.shape[0]):
        if status is None or status[i] == 0:
            out[i] = stats_image(labels[i], n_ids)
    return out


def to_raw(public, out_w, out_h):
    p = np.asarray(public, np.int64)
    raw = np.stack([p[..., 0], p[..., 3], p[..., 4], out_w - p[..., 1], out_h - p[..., 2]], axis=-1)
    raw[p[..., 0] == 0] = 0
    return raw.astype(np.uint32)


def to_public(raw, out_w, out_h):
    r = np.asarray(raw).astype(np.int64)
    pub = np.stack([r[..., 0], out_w - r[..., 3], out_h - r[..., 4], r[..., 1], r[..., 2]], axis=-1)
    pub[r[..., 0] == 0] = 0
    return pub
