"""TEST HELPER for the spec-complete PNG path (include/decode_png.h: debig_png_decode_batch).

numpy + the stdlib's zlib only:
  * encode(...)  -- a PNG encoder for any (colour type, bit depth, interlace, tRNS, filter type per row, IDAT split)
                    combination, with stored / fixed / dynamic DEFLATE blocks;
  * decode(data) -- a straightforward reference decoder of the rules debig_png_decode_batch documents:
                    -> (status, rgba (h, w, 4) uint8 or None, info dict).
  * pixels(raw, ...) -- the de-filter and conversion steps of decode on their own (tests/png_damage.py);
  * scanlines(...) / tasks_for(...) -- the scanline stream and the Adam7 pass geometry (emulator tests).
"""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"

# status codes (include/decode_png.h: DEBIG_PNG_*)
OK, E_SIGNATURE, E_CHUNK, E_IHDR, E_CRC, E_ZLIB, E_INFLATE, E_ADLER, E_DATA_SHORT, E_DATA_LONG, E_FILTER, E_PALETTE, \
    E_OUTPUT = range(13)

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def passes(w, h, interlace):
    """[(x0, y0, dx, dy, w_p, h_p)] of the non-empty sub-images"""
    geo = ADAM7 if interlace else ((0, 0, 1, 1),)
    out = []
    for x0, y0, dx, dy in geo:
        wp = (w - x0 + dx - 1) // dx if w > x0 else 0
        hp = (h - y0 + dy - 1) // dy if h > y0 else 0
        if wp and hp:
            out.append((x0, y0, dx, dy, wp, hp))
    return out


def row_bytes(wp, ct, depth):
    return (wp * CHANNELS[ct] * depth + 7) // 8


def bpp_f(ct, depth):
    return max(1, CHANNELS[ct] * depth // 8)


def scanline_size(w, h, ct, depth, interlace):
    return sum(hp * (1 + row_bytes(wp, ct, depth)) for _, _, _, _, wp, hp in passes(w, h, interlace))


# ------------------------------------------------------------------------------------------------ encoder
def _pack_row(samples, depth):
    """samples: 1-D array of raw sample values of one row -> bytes"""
    if depth == 16:
        return samples.astype(">u2").tobytes()
    if depth == 8:
        return samples.astype(np.uint8).tobytes()
    per = 8 // depth
    s = np.zeros(((len(samples) + per - 1) // per) * per, dtype=np.uint32)
    s[: len(samples)] = samples
    s = s.reshape(-1, per)
    b = np.zeros(len(s), dtype=np.uint32)
    for k in range(per):
        b |= s[:, k] << (8 - depth * (k + 1))
    return b.astype(np.uint8).tobytes()


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def _filter_row(ft, raw, prev, bpp):
    out = bytearray(len(raw))
    for i in range(len(raw)):
        a = raw[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        if ft == 0:
            p = 0
        elif ft == 1:
            p = a
        elif ft == 2:
            p = b
        elif ft == 3:
            p = (a + b) >> 1
        else:
            p = _paeth(a, b, c)
        out[i] = (raw[i] - p) & 0xFF
    return bytes(out)


def chunk(typ, data):
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data) & 0xFFFFFFFF)


def scanlines(samples, ct, depth, interlace=0, filters=None):
    """the decompressed scanline stream.  samples: (h, w, channels) raw sample values (palette: indices).
    filters: None (row y of pass p gets (y + p) % 5), an int (every row), or a callable (pass, y) -> type"""
    samples = np.asarray(samples)
    if samples.ndim == 2:
        samples = samples[:, :, None]
    h, w, _ = samples.shape
    bpp = bpp_f(ct, depth)
    out = bytearray()
    for p, (x0, y0, dx, dy, wp, hp) in enumerate(passes(w, h, interlace)):
        sub = samples[y0::dy, x0::dx]
        prev = bytes(row_bytes(wp, ct, depth))
        for y in range(hp):
            raw = _pack_row(sub[y].reshape(-1), depth)
            if filters is None:
                ft = (y + p) % 5
            elif callable(filters):
                ft = filters(p, y)
            else:
                ft = int(filters)
            out.append(ft)
            out += _filter_row(ft, raw, prev, bpp)
            prev = raw
    return bytes(out)


def zlib_stream(data, mode="default"):
    """mode: 'stored' (level 0), 'fixed' (Z_FIXED), 'default' (dynamic blocks)"""
    if mode == "stored":
        co = zlib.compressobj(0)
    elif mode == "fixed":
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    else:
        co = zlib.compressobj(6)
    return co.compress(data) + co.flush()


def encode(samples, ct, depth, interlace=0, trns=None, palette=None, filters=None, idat_split=None, mode="default",
           zdata=None, extra_before_idat=(), ihdr=None):
    """a PNG file.  trns: bytes of the tRNS chunk body or None; palette: list of (r, g, b) or None; idat_split: sizes
    of the IDAT chunks (the rest goes into the last one); zdata: the zlib stream itself (overrides the encoding);
    ihdr: a replacement IHDR body."""
    samples = np.asarray(samples)
    if samples.ndim == 2:
        samples = samples[:, :, None]
    h, w, _ = samples.shape
    if zdata is None:
        zdata = zlib_stream(scanlines(samples, ct, depth, interlace, filters), mode)
    body = ihdr if ihdr is not None else struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, interlace)
    out = SIG + chunk(b"IHDR", body)
    for typ, data in extra_before_idat:
        out += chunk(typ, data)
    if palette is not None:
        out += chunk(b"PLTE", bytes(np.asarray(palette, dtype=np.uint8).reshape(-1)))
    if trns is not None:
        out += chunk(b"tRNS", trns)
    pieces = []
    rest = zdata
    for s in idat_split or ():
        pieces.append(rest[:s])
        rest = rest[s:]
    pieces.append(rest)
    for piece in pieces:
        out += chunk(b"IDAT", piece)
    return out + chunk(b"IEND", b"")


def random_image(rng, w, h, ct, depth, n_pal=None):
    """random raw samples for (ct, depth); palette indices below n_pal"""
    ch = CHANNELS[ct]
    if ct == 3:
        top = n_pal if n_pal is not None else 1 << depth
        return rng.integers(0, top, size=(h, w, 1), dtype=np.uint16).astype(np.uint8)
    top = 1 << depth
    s = rng.integers(0, top, size=(h, w, ch), dtype=np.uint32)
    return s.astype(np.uint16 if depth == 16 else np.uint8)


# ------------------------------------------------------------------------------------------------ decoder
def _unfilter(data, pos, wp, hp, rb, bpp):
    """-> (rows (hp, rb) uint8, first bad row or None, new pos)"""
    rows = np.zeros((hp, rb), dtype=np.uint8)
    prev = [0] * rb
    for y in range(hp):
        ft = data[pos]
        if ft > 4:
            return rows, y, pos
        f = data[pos + 1: pos + 1 + rb]
        pos += 1 + rb
        cur = [0] * rb
        if ft == 0:
            cur = list(f)
        elif ft == 2:
            cur = [(f[i] + prev[i]) & 0xFF for i in range(rb)]
        else:
            for i in range(rb):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) >> 1
                else:
                    p = _paeth(a, b, prev[i - bpp] if i >= bpp else 0)
                cur[i] = (f[i] + p) & 0xFF
        rows[y] = cur
        prev = cur
    return rows, None, pos


def _samples(rows, wp, ct, depth):
    """raw rows -> (hp, wp, channels) samples at full depth"""
    ch = CHANNELS[ct]
    if depth == 16:
        return rows[:, : wp * ch * 2].reshape(len(rows), -1).view(">u2").astype(np.uint32).reshape(len(rows), wp, ch)
    if depth == 8:
        return rows[:, : wp * ch].astype(np.uint32).reshape(len(rows), wp, ch)
    bits = np.unpackbits(rows, axis=1)
    bits = bits[:, : wp * depth].reshape(len(rows), wp, depth)
    v = np.zeros((len(rows), wp), dtype=np.uint32)
    for k in range(depth):
        v = (v << 1) | bits[:, :, k]
    return v.reshape(len(rows), wp, 1)


def _to_rgba(s, ct, depth, key, pal):
    """samples -> RGBA8; returns (rgba, palette index out of range)"""
    hp, wp, _ = s.shape
    rgba = np.zeros((hp, wp, 4), dtype=np.uint8)
    hi = (s >> 8) if depth == 16 else s
    if ct == 3:
        idx = s[:, :, 0]
        bad = bool((idx >= len(pal)).any())
        full = np.zeros((256, 4), dtype=np.uint8)
        full[: len(pal)] = pal
        return full[np.minimum(idx, 255)], bad
    if ct in (0, 4):
        g = hi[:, :, 0]
        if depth < 8:
            g = g * {1: 255, 2: 85, 4: 17}[depth]
        rgba[:, :, 0] = rgba[:, :, 1] = rgba[:, :, 2] = g
        if ct == 4:
            rgba[:, :, 3] = hi[:, :, 1]
        else:
            rgba[:, :, 3] = 255
            if key is not None:
                rgba[:, :, 3][s[:, :, 0] == key[0]] = 0
    else:
        rgba[:, :, :3] = hi[:, :, :3]
        if ct == 6:
            rgba[:, :, 3] = hi[:, :, 3]
        else:
            rgba[:, :, 3] = 255
            if key is not None:
                m = (s[:, :, 0] == key[0]) & (s[:, :, 1] == key[1]) & (s[:, :, 2] == key[2])
                rgba[:, :, 3][m] = 0
    return rgba, False


def info(data):
    """-> (status, info dict) from the signature, IHDR and the chunks up to the first IDAT (debig_png_info_get)"""
    st, inf, _ = _walk(data, info_only=True)
    return st, inf


def _walk(data, info_only=False):
    inf = {"width": 0, "height": 0, "bit_depth": 0, "color_type": 0, "interlace": 0, "has_trns": 0}
    if len(data) < 8 or data[:8] != SIG:
        return E_SIGNATURE, inf, None
    pos = 8
    seen_ihdr = seen_plte = seen_idat = idat_done = False
    pal, trns, key, chunks, idat = None, None, None, [], []
    while True:
        if pos + 8 > len(data):
            return E_CHUNK, inf, None
        ln = struct.unpack(">I", data[pos: pos + 4])[0]
        typ = data[pos + 4: pos + 8]
        if ln > 0x7FFFFFFF or pos + 12 + ln > len(data):
            return E_CHUNK, inf, None
        body = data[pos + 8: pos + 8 + ln]
        crc = struct.unpack(">I", data[pos + 8 + ln: pos + 12 + ln])[0]
        if not seen_ihdr and typ != b"IHDR":
            return E_CHUNK, inf, None
        if typ == b"IHDR":
            if seen_ihdr:
                return E_CHUNK, inf, None
            if ln != 13:
                return E_IHDR, inf, None
            w, h, depth, ct, comp, filt, il = struct.unpack(">IIBBBBB", body)
            if not (1 <= w <= 0x7FFFFFFF and 1 <= h <= 0x7FFFFFFF) or ct not in DEPTHS or depth not in DEPTHS[ct] \
                    or comp != 0 or filt != 0 or il > 1:
                return E_IHDR, inf, None
            inf.update(width=w, height=h, bit_depth=depth, color_type=ct, interlace=il)
            seen_ihdr = True
        elif typ == b"IDAT":
            if idat_done:
                return E_CHUNK, inf, None
            if info_only:
                break
            seen_idat = True
            idat.append(body)
        else:
            if seen_idat:
                idat_done = True
            if typ == b"IEND":
                chunks.append((typ + body, crc))
                break
            if typ == b"PLTE":
                if seen_plte or seen_idat or inf["color_type"] in (0, 4):
                    return E_CHUNK, inf, None
                seen_plte = True
                if inf["color_type"] == 3:
                    if ln % 3 or not 3 <= ln <= 768:
                        return E_PALETTE, inf, None
                    pal = np.full((ln // 3, 4), 255, dtype=np.uint8)
                    pal[:, :3] = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3)
            elif typ == b"tRNS":
                if not seen_idat:
                    trns = (body, pal is not None)
            elif not (typ[0] & 0x20):
                return E_CHUNK, inf, None
        chunks.append((typ + body, crc))
        pos += 12 + ln
    ct = inf["color_type"]
    if ct == 3 and pal is None:
        return E_CHUNK, inf, None
    if trns is not None:
        body, after_plte = trns
        if ct == 3 and after_plte and len(body) <= len(pal):
            pal[: len(body), 3] = np.frombuffer(body, dtype=np.uint8)
            inf["has_trns"] = 1
        elif ct == 0 and len(body) == 2:
            key = struct.unpack(">H", body)
            inf["has_trns"] = 1
        elif ct == 2 and len(body) == 6:
            key = struct.unpack(">HHH", body)
            inf["has_trns"] = 1
    if info_only:
        return OK, inf, None
    if not idat:
        return E_CHUNK, inf, None
    return OK, inf, (pal, key, chunks, b"".join(idat))


def decode(data, out_cap=None):
    """-> (status, rgba (h, w, 4) or None, info)"""
    st, inf, rest = _walk(bytes(data))
    if st != OK:
        return st, None, inf
    pal, key, chunks, z = rest
    w, h, ct, depth, il = inf["width"], inf["height"], inf["color_type"], inf["bit_depth"], inf["interlace"]
    if len(z) < 2 or (z[0] & 15) != 8 or (z[0] >> 4) > 7 or ((z[0] << 8) | z[1]) % 31 or (z[1] & 0x20):
        return E_ZLIB, None, inf
    if out_cap is not None and out_cap < 4 * w * h:
        return E_OUTPUT, None, inf
    for body, crc in chunks:
        if zlib.crc32(body) & 0xFFFFFFFF != crc:
            return E_CRC, None, inf
    size = scanline_size(w, h, ct, depth, il)
    d = zlib.decompressobj(-15)
    try:
        raw = d.decompress(z[2:], size + 1)
    except zlib.error:
        return E_INFLATE, None, inf
    if len(raw) > size:
        return E_DATA_LONG, None, inf
    if not d.eof:
        return E_INFLATE, None, inf
    if len(raw) < size:
        return E_DATA_SHORT, None, inf
    tail = d.unused_data
    if len(tail) < 4 or struct.unpack(">I", tail[:4])[0] != zlib.adler32(raw) & 0xFFFFFFFF:
        return E_ADLER, None, inf
    st, out = pixels(raw, inf, pal, key)
    return st, out, inf


def pixels(raw, inf, pal, key):
    """the scanline stream (exactly scanline_size bytes) -> (OK, rgba (h, w, 4)) or (E_FILTER / E_PALETTE, None): the
    last two steps of decode (a filter error anywhere outranks a palette error)"""
    w, h, ct, depth, il = inf["width"], inf["height"], inf["color_type"], inf["bit_depth"], inf["interlace"]
    out = np.zeros((h, w, 4), dtype=np.uint8)
    pos = 0
    parts = []
    for x0, y0, dx, dy, wp, hp in passes(w, h, il):
        rb = row_bytes(wp, ct, depth)
        rows, bad, pos = _unfilter(raw, pos, wp, hp, rb, bpp_f(ct, depth))
        if bad is not None:
            return E_FILTER, None
        parts.append((x0, y0, dx, dy, _samples(rows, wp, ct, depth)))
    for x0, y0, dx, dy, s in parts:
        rgba, bad = _to_rgba(s, ct, depth, key, pal)
        if bad:
            return E_PALETTE, None
        out[y0::dy, x0::dx] = rgba
    return OK, out


def full_palette(pal_rgb, trns=b""):
    """256 RGBA dwords as the kernel takes them (entries past the palette 0)"""
    p = np.zeros((256, 4), dtype=np.uint8)
    n = len(pal_rgb)
    p[:n, :3] = np.asarray(pal_rgb, dtype=np.uint8)
    p[:n, 3] = 255
    if trns:
        p[: len(trns), 3] = np.frombuffer(trns, dtype=np.uint8)
    return p
