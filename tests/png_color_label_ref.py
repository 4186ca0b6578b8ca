"""TEST HELPER for the colour-label decode (include/decode_png.h: debig_png_decode_batch_color_labels): the numpy restatement.

  * rgb(data)                 -- (status, (h, w, 3) uint8 or None, info): the RGB8 pixels of tests/png_out_format_ref.py, with
                                 E_LABEL for a 16-bit file as soon as IHDR has been read;
  * pack(px)                  -- R | G << 8 | B << 16 per pixel, uint32;
  * gather(px, size, box, colors, missing, dtype) -- crop and pick by png_label_ref.index, pack, look every colour up in a
                                 Python dict (colors None: the packed colour itself) -> ((H, W) array of dtype, unmatched);
  * slot(key, slots), slots_for(n), table(keys, values) -- the lookup table of include/debig_hip.h restated: slot function,
                                 slot count, linear probing in insertion order.
It never reads the code under test.
"""
import numpy as np

import png_label_ref as LR
import png_out_format_ref as F
import png_spec_ref as R

E_BOX, E_LABEL = LR.E_BOX, LR.E_LABEL
DTYPES = LR.DTYPES
CMAP_MAX, MAX_SLOTS, EMPTY = 2048, 4096, 0xFFFFFFFF


def rgb(data):
    """-> (status, (h, w, 3) uint8 or None, info)"""
    st, inf, _ = R._walk(bytes(data))
    if inf["width"] and inf["bit_depth"] == 16:  # decided as soon as IHDR has been read
        return E_LABEL, None, inf
    st, px, inf = F.decode(data, F.RGB | F.D8)
    return st, px, inf


def pack(px):
    p = np.asarray(px).astype(np.uint32)
    return p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)


def gather(px, size, box=None, colors=None, missing=-1, dtype="int64"):
    """px (h, w, 3) uint8; colors: None or a dict {packed key: value} -> ((H, W) of dtype, number of elements not in colors)"""
    h, w = px.shape[:2]
    H, W = size
    x, y, bw, bh = (0, 0, w, h) if box is None or (box[2] == 0 and box[3] == 0) else box
    key = pack(px[y + LR.index(bh, H)][:, x + LR.index(bw, W)])
    if colors is None:
        return key.astype(np.int64).astype(DTYPES[dtype]), 0
    out = np.empty(key.shape, dtype=np.int64)
    miss = 0
    for k in np.unique(key):
        m = key == k
        if int(k) in colors:
            out[m] = colors[int(k)]
        else:
            out[m] = missing
            miss += int(m.sum())
    return out.astype(DTYPES[dtype]), miss


def slot(key, slots):
    return (((key * 0x9E3779B1) & 0xFFFFFFFF) >> 20) & (slots - 1)


def slots_for(n):
    s = 2
    while s < 2 * n:
        s *= 2
    return s


def table(keys, values, slots=None):
    """-> (slots, 2) uint32: (key, value bits) per slot, EMPTY keys where unused"""
    slots = slots or slots_for(len(keys))
    t = np.zeros((slots, 2), dtype=np.uint32)
    t[:, 0] = EMPTY
    for k, v in zip(keys, values):
        s = slot(int(k), slots)
        while t[s, 0] != EMPTY:
            assert t[s, 0] != k, "two equal keys"
            s = (s + 1) & (slots - 1)
        t[s] = (int(k), int(v) & 0xFFFFFFFF)
    return t
