"""TEST HELPER for the label decode (include/decode_png.h: debig_png_decode_batch_labels): the numpy restatement.

  * labels(data, dtype, lut) -- (status, (h, w) uint32 raw labels or None, info dict): the palette index (colour type 3) or
                                the raw grey sample (colour type 0) of every pixel, by the chunk walk, the inflate / Adler /
                                CRC checks and the de-filter of tests/png_spec_ref.py, scattered by Adam7 pass;
  * index(cl, L)             -- the source index of every output coordinate: ((2X + 1) cl) div 2L;
  * gather(lab, size, box, lut, dtype) -- crop, pick, remap and widen -> (H, W) array of dtype.
"""
import struct
import zlib

import numpy as np

import png_spec_ref as R

E_BOX, E_LABEL = 14, 15
DTYPES = {"uint8": np.uint8, "uint16": np.uint16, "int32": np.int32, "int64": np.int64}


def label_error(info, dtype="int64", lut=None):
    """the E_LABEL rule on a valid IHDR: colour type 2, 4 or 6; a 16-bit file with dtype uint8; a 16-bit file with a lut"""
    return info["color_type"] not in (0, 3) or (info["bit_depth"] == 16 and (dtype == "uint8" or lut is not None))


def labels(data, dtype="int64", lut=None):
    """-> (status, (h, w) uint32 or None, info); dtype and lut only decide E_LABEL"""
    st, inf, rest = R._walk(bytes(data))
    if inf["width"] and label_error(inf, dtype, lut):  # decided as soon as IHDR has been read
        return E_LABEL, None, inf
    if st != R.OK:
        return st, None, inf
    pal, _, chunks, z = rest
    w, h, ct, depth, il = inf["width"], inf["height"], inf["color_type"], inf["bit_depth"], inf["interlace"]
    if len(z) < 2 or (z[0] & 15) != 8 or (z[0] >> 4) > 7 or ((z[0] << 8) | z[1]) % 31 or (z[1] & 0x20):
        return R.E_ZLIB, None, inf
    for body, crc in chunks:
        if zlib.crc32(body) & 0xFFFFFFFF != crc:
            return R.E_CRC, None, inf
    size = R.scanline_size(w, h, ct, depth, il)
    d = zlib.decompressobj(-15)
    try:
        raw = d.decompress(z[2:], size + 1)
    except zlib.error:
        return R.E_INFLATE, None, inf
    if len(raw) > size:
        return R.E_DATA_LONG, None, inf
    if not d.eof:
        return R.E_INFLATE, None, inf
    if len(raw) < size:
        return R.E_DATA_SHORT, None, inf
    tail = d.unused_data
    if len(tail) < 4 or struct.unpack(">I", tail[:4])[0] != zlib.adler32(raw) & 0xFFFFFFFF:
        return R.E_ADLER, None, inf
    out = np.zeros((h, w), dtype=np.uint32)
    pos = 0
    for x0, y0, dx, dy, wp, hp in R.passes(w, h, il):
        rows, bad, pos = R._unfilter(raw, pos, wp, hp, R.row_bytes(wp, ct, depth), R.bpp_f(ct, depth))
        if bad is not None:
            return R.E_FILTER, None, inf
        out[y0::dy, x0::dx] = R._samples(rows, wp, ct, depth)[:, :, 0]
    if ct == 3 and (out >= len(pal)).any():
        return R.E_PALETTE, None, inf
    return R.OK, out, inf


def index(cl, L):
    """source index inside a crop of length cl for every output coordinate 0 .. L - 1 (Python integers: no overflow)"""
    return np.array([((2 * X + 1) * cl) // (2 * L) for X in range(L)], dtype=np.int64)


def box_error(box, w, h):
    """the box rules of debig_png_decode_batch_tensor without a scale limit"""
    if box is None or (box[2] == 0 and box[3] == 0):
        return False
    x, y, bw, bh = box
    return bw == 0 or bh == 0 or x + bw > w or y + bh > h


def gather(lab, size, box=None, lut=None, dtype="int64"):
    """lab (h, w) raw labels -> (H, W) of dtype: element (Y, X) = lut[lab[by + sy[Y], bx + sx[X]]]"""
    h, w = lab.shape
    H, W = size
    x, y, bw, bh = (0, 0, w, h) if box is None or (box[2] == 0 and box[3] == 0) else box
    v = lab[y + index(bh, H)][:, x + index(bw, W)].astype(np.int64)
    if lut is not None:
        v = np.asarray(lut, dtype=np.int64)[v]
    return v.astype(DTYPES[dtype])
