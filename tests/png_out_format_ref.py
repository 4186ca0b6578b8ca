"""TEST HELPER: the output formats of debig_png_decode_batch_fmt (include/decode_png.h), in numpy.

  * resolve(ct, depth, has_trns, out_format) -> (layout, bits): NATIVE layout / depth resolved per image;
  * layout(w, h, ct, depth, has_trns, out_format) -> (channels, bytes_per_sample, nbytes), 0s for a bad format;
  * convert(s, ct, depth, key, pal, out_format) -> (h, w, channels) uint8 / uint16 from the raw samples of
    png_spec_ref._samples (palette: indices);
  * decode(data, out_format) -> (status, pixels or None, info), png_spec_ref.decode's statuses.
"""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_spec_ref as R  # noqa: E402

RGBA, RGB, GRAY, GRAY_ALPHA, NATIVE = range(5)
D8, D16, D_NATIVE = 0x00, 0x10, 0x20
LAYOUT_CHANNELS = {RGBA: 4, RGB: 3, GRAY: 1, GRAY_ALPHA: 2}
# every valid out_format
FORMATS = [lay | d for d in (D8, D16, D_NATIVE) for lay in (RGBA, RGB, GRAY, GRAY_ALPHA, NATIVE)]
MODES = {RGBA: "rgba", RGB: "rgb", GRAY: "gray", GRAY_ALPHA: "gray_alpha", NATIVE: "native"}
DEPTHS = {D8: 8, D16: 16, D_NATIVE: "native"}


def valid(out_format):
    return out_format in FORMATS


def resolve(ct, depth, has_trns, out_format):
    """-> (concrete layout 0..3, output bits 8 / 16)"""
    lay, d = out_format & 15, out_format & 0x30
    if lay == NATIVE:
        lay = {0: GRAY_ALPHA if has_trns else GRAY, 4: GRAY_ALPHA, 2: RGBA if has_trns else RGB,
               3: RGBA if has_trns else RGB, 6: RGBA}[ct]
    if d == D_NATIVE:
        d = D16 if depth == 16 else D8
    return lay, 16 if d == D16 else 8


def layout(w, h, ct, depth, has_trns, out_format):
    if not valid(out_format):
        return 0, 0, 0
    lay, bits = resolve(ct, depth, has_trns, out_format)
    ch, bs = LAYOUT_CHANNELS[lay], bits // 8
    return ch, bs, w * h * ch * bs


def source16(s, ct, depth, key, pal):
    """raw samples -> (R, G, B, A) as uint32 at 16 bits (steps 1 and 2 of the contract with D = 16: 8-bit values
    times 257; sub-byte grey scaled to 8 bits first)"""
    s = np.asarray(s).astype(np.uint32)
    if s.ndim == 2:
        s = s[:, :, None]
    hp, wp, _ = s.shape
    out = np.zeros((hp, wp, 4), dtype=np.uint32)
    if ct == 3:
        full = np.zeros((256, 4), dtype=np.uint32)
        full[: len(pal)] = np.asarray(pal, dtype=np.uint32)
        out[:] = full[np.minimum(s[:, :, 0], 255)] * 257
        return out
    v = s if depth == 16 else s * {1: 255, 2: 85, 4: 17, 8: 1}[depth] * 257
    if ct in (0, 4):
        out[:, :, 0] = out[:, :, 1] = out[:, :, 2] = v[:, :, 0]
        if ct == 4:
            out[:, :, 3] = v[:, :, 1]
        else:
            out[:, :, 3] = 65535
            if key is not None:
                out[:, :, 3][s[:, :, 0] == key[0]] = 0
    else:
        out[:, :, :3] = v[:, :, :3]
        if ct == 6:
            out[:, :, 3] = v[:, :, 3]
        else:
            out[:, :, 3] = 65535
            if key is not None:
                m = (s[:, :, 0] == key[0]) & (s[:, :, 1] == key[1]) & (s[:, :, 2] == key[2])
                out[:, :, 3][m] = 0
    return out


def convert(s, ct, depth, key, pal, out_format, has_trns=None):
    """raw samples (png_spec_ref._samples; palette: indices, pal: (n, 4) RGBA with tRNS folded in) -> pixels"""
    if has_trns is None:
        has_trns = key is not None if ct in (0, 2) else ct == 3 and bool((np.asarray(pal)[:, 3] != 255).any())
    lay, bits = resolve(ct, depth, has_trns, out_format)
    p = source16(s, ct, depth, key, pal)
    if bits == 8:
        p = p >> 8  # 16 -> 8: the high byte; 8 -> 16 -> 8 is the identity
    r, g, b, a = p[:, :, 0], p[:, :, 1], p[:, :, 2], p[:, :, 3]
    y = (6968 * r + 23434 * g + 2366 * b + 16384) >> 15
    chans = {RGBA: (r, g, b, a), RGB: (r, g, b), GRAY: (y,), GRAY_ALPHA: (y, a)}[lay]
    return np.stack(chans, axis=2).astype(np.uint16 if bits == 16 else np.uint8)


def decode(data, out_format=0):
    """-> (status, pixels (h, w, channels) or None, info), by png_spec_ref's rules"""
    st, _, inf = R.decode(data)
    if st != R.OK:
        return st, None, inf
    _, _, rest = R._walk(bytes(data))
    pal, key, _, z = rest
    w, h, ct, depth, il = inf["width"], inf["height"], inf["color_type"], inf["bit_depth"], inf["interlace"]
    raw = zlib.decompressobj(-15).decompress(z[2:])
    lay, bits = resolve(ct, depth, inf["has_trns"], out_format)
    out = np.zeros((h, w, LAYOUT_CHANNELS[lay]), dtype=np.uint16 if bits == 16 else np.uint8)
    pos = 0
    for x0, y0, dx, dy, wp, hp in R.passes(w, h, il):
        rows, _, pos = R._unfilter(raw, pos, wp, hp, R.row_bytes(wp, ct, depth), R.bpp_f(ct, depth))
        s = R._samples(rows, wp, ct, depth)
        out[y0::dy, x0::dx] = convert(s, ct, depth, key, pal, out_format, has_trns=inf["has_trns"])
    return R.OK, out, inf
