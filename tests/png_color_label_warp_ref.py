"""TEST HELPER for the affine warp of colour-coded label maps (include/decode_png.h: debig_png_decode_batch_color_labels_warp):
the numpy restatement.  It composes the pick of tests/png_warp_ref.py with the lookup of tests/png_color_label_ref.py.

  * warp_color_labels(px, size, m, mode, border_label, box, colors, missing, dtype) -- px (h, w, 3) uint8 decoded RGB8 pixels,
        m the six quantised integers -> ((H, W) array of dtype, unmatched):
          - the pick is (jx, jy) = png_warp_ref.picks(size, m), compared against the crop as Python / int64 integers;
          - inside the crop, or anywhere under CLAMP (indices clamped to [0, cl - 1]): the packed colour (colors None) or its
            value in `colors` (a dict {packed key: value}), else `missing`;
          - outside under CONSTANT: border_label as it is;
          - unmatched: the elements that took `missing` through the map.  A border element under CONSTANT is never one of them,
            even when border_label == missing; a clamped pick counts like any other; 0 when colors is None.
It never reads the code under test.
"""
import numpy as np

import png_color_label_ref as CR
import png_warp_ref as WR

CONSTANT, CLAMP = WR.CONSTANT, WR.CLAMP
E_WARP = WR.E_WARP
DTYPES = CR.DTYPES


def warp_color_labels(px, size, m, mode=CONSTANT, border_label=0, box=None, colors=None, missing=-1, dtype="int64"):
    if box is not None and (box[2] or box[3]):
        x, y, w, h = box
        px = px[y:y + h, x:x + w]
    h, w = px.shape[:2]
    jx, jy = WR.picks(size, m)
    inside = (jx >= 0) & (jx < w) & (jy >= 0) & (jy < h)
    key = CR.pack(px[np.clip(jy, 0, h - 1), np.clip(jx, 0, w - 1)])
    keep = inside if mode == CONSTANT else np.ones_like(inside)
    out = key.astype(np.int64)
    miss = 0
    if colors is not None:
        for k in np.unique(key):
            sel = key == k
            if int(k) in colors:
                out[sel] = colors[int(k)]
            else:
                out[sel] = missing
                miss += int((sel & keep).sum())
    out[~keep] = border_label
    return out.astype(DTYPES[dtype]), miss
