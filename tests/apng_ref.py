"""APNG reference (CPU): an encoder on top of tests/png_spec_ref.py and a decoder that rebuilds every frame as a standalone
PNG (IHDR at the frame's size + the file's PLTE / tRNS + one IDAT holding the frame's stream + IEND), decodes it with
png_spec_ref.decode and composites with the rules of include/decode_png.h in numpy."""
import struct

import numpy as np

import png_spec_ref as R

E_ANIM = 13
NONE, BACKGROUND, PREVIOUS = 0, 1, 2
SOURCE, OVER = 0, 1


def actl(num_frames, num_plays=0):
    return (b"acTL", struct.pack(">II", num_frames, num_plays))


def fctl(seq, w, h, x=0, y=0, delay_num=1, delay_den=10, dispose=0, blend=0):
    return (b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, x, y, delay_num, delay_den, dispose, blend))


def fdat(seq, data):
    return (b"fdAT", struct.pack(">I", seq) + data)


def assemble(chunks):
    """[(type, body)] -> the file (fresh CRCs)"""
    return R.SIG + b"".join(R.chunk(t, d) for t, d in chunks)


def renumber(chunks):
    """sequence numbers 0, 1, 2, ... over the fcTL and fdAT chunks, in order"""
    out, seq = [], 0
    for t, d in chunks:
        if t in (b"fcTL", b"fdAT") and len(d) >= 4:
            d = struct.pack(">I", seq) + d[4:]
            seq += 1
        out.append((t, d))
    return out


def frame(samples, x=0, y=0, dispose=NONE, blend=SOURCE, delay=(1, 10)):
    """one frame: raw samples (h, w[, channels]) as png_spec_ref takes them (palette: indices) and its fcTL fields"""
    return {"samples": np.asarray(samples), "x": x, "y": y, "dispose": dispose, "blend": blend, "delay": delay}


def apng_chunks(frames, ct, depth, interlace=0, palette=None, trns=None, default=None, num_plays=0, fdat_split=None,
                mode="default", zdata=None):
    """the chunk list of an APNG.  default: None -> the IDAT image is frame 0 (the canvas is its size), else the raw
    samples of a default image that is not a frame (the canvas is its size).  fdat_split: sizes of the first fdAT
    pieces of every later frame's stream (the rest goes into the last one).  zdata: {frame index: zlib stream} to use
    instead of the encoded one."""
    if default is None:
        h, w = frames[0]["samples"].shape[:2]
    else:
        h, w = np.asarray(default).shape[:2]
    ch = [(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, interlace)), actl(len(frames), num_plays)]
    if palette is not None:
        ch.append((b"PLTE", bytes(np.asarray(palette, dtype=np.uint8).reshape(-1))))
    if trns is not None:
        ch.append((b"tRNS", trns))
    seq = 0

    def stream(k, f):
        if zdata is not None and k in zdata:
            return zdata[k]
        return R.zlib_stream(R.scanlines(f["samples"], ct, depth, interlace), mode)

    def fc(f):
        nonlocal seq
        fh, fw = f["samples"].shape[:2]
        c = fctl(seq, fw, fh, f["x"], f["y"], f["delay"][0], f["delay"][1], f["dispose"], f["blend"])
        seq += 1
        return c

    if default is None:
        ch += [fc(frames[0]), (b"IDAT", stream(0, frames[0]))]
    else:
        ch.append((b"IDAT", R.zlib_stream(R.scanlines(default, ct, depth, interlace), mode)))
    for k, f in enumerate(frames[1:] if default is None else frames, 1 if default is None else 0):
        ch.append(fc(f))
        z = stream(k, f)
        pieces = []
        for s in fdat_split or ():
            pieces.append(z[:s])
            z = z[s:]
        pieces.append(z)
        for p in pieces:
            ch.append(fdat(seq, p))
            seq += 1
    ch.append((b"IEND", b""))
    return ch


def encode(frames, ct, depth, **kw):
    return assemble(apng_chunks(frames, ct, depth, **kw))


# ------------------------------------------------------------------------------------------------ decoder
def _chunks(data):
    """[(type, body)] up to IEND (of a file whose walk passed)"""
    out, pos = [], 8
    while True:
        ln = struct.unpack(">I", data[pos: pos + 4])[0]
        t = data[pos + 4: pos + 8]
        out.append((t, data[pos + 8: pos + 8 + ln]))
        pos += 12 + ln
        if t == b"IEND":
            return out


def anim_walk(data, inf):
    """the animation rules over a file whose walk passed -> (status, info additions, frame streams or None)"""
    ch = _chunks(data)
    W, H = inf["width"], inf["height"]
    ai = {"num_frames": 1, "num_plays": 0, "default_is_frame": 1, "frames": []}
    idat = b"".join(b for t, b in ch if t == b"IDAT")
    if not any(t == b"acTL" for t, _ in ch):
        ai["frames"] = [dict(x=0, y=0, width=W, height=H, delay_num=0, delay_den=0, dispose=0, blend=0)]
        return R.OK, ai, [idat]
    ai.update(num_frames=0, default_is_frame=0)
    streams = []
    seen_idat, n_actl, seq, n_before, cur_after, cur_fdat = False, 0, 0, 0, False, 0
    for t, b in ch:
        if t == b"IDAT":
            if not seen_idat and streams:
                ai["default_is_frame"] = 1
                streams[0] = idat
            seen_idat = True
        elif t == b"acTL":
            if seen_idat or n_actl or len(b) != 8:
                return E_ANIM, ai, None
            n_actl += 1
            ai["num_frames"], ai["num_plays"] = struct.unpack(">II", b)
            if ai["num_frames"] == 0:
                return E_ANIM, ai, None
        elif t == b"fcTL":
            if len(b) != 26:
                return E_ANIM, ai, None
            s, w, h, x, y, dn, dd, dop, bop = struct.unpack(">IIIIIHHBB", b)
            if s != seq:
                return E_ANIM, ai, None
            seq += 1
            if w == 0 or h == 0 or x + w > W or y + h > H or dop > 2 or bop > 1:
                return E_ANIM, ai, None
            if not seen_idat:
                if n_before or x or y or w != W or h != H:
                    return E_ANIM, ai, None
                n_before += 1
            elif cur_after and cur_fdat == 0:
                return E_ANIM, ai, None
            ai["frames"].append(dict(x=x, y=y, width=w, height=h, delay_num=dn, delay_den=dd, dispose=dop, blend=bop))
            streams.append(b"")
            cur_after, cur_fdat = seen_idat, 0
        elif t == b"fdAT":
            if not seen_idat or len(b) < 4 or not cur_after or struct.unpack(">I", b[:4])[0] != seq:
                return E_ANIM, ai, None
            seq += 1
            cur_fdat += 1
            streams[-1] += b[4:]
    if cur_after and cur_fdat == 0:
        return E_ANIM, ai, None
    if len(ai["frames"]) != ai["num_frames"]:
        return E_ANIM, ai, None
    return R.OK, ai, streams


def over(s, d):
    """s OVER d on uint8 (..., 4) arrays: the integer rule of include/decode_png.h"""
    s = s.astype(np.uint32)
    d = d.astype(np.uint32)
    sa, da = s[..., 3:4], d[..., 3:4]
    u = sa * 255
    v = (255 - sa) * da
    al = u + v
    c = (s[..., :3] * u + d[..., :3] * v) // np.maximum(al, 1)
    out = np.concatenate([c, al // 255], axis=-1)
    out = np.where(sa == 255, s, np.where(sa == 0, d, out))
    return out.astype(np.uint8)


def composite(pixels, frames, W, H):
    """RGBA8 frame pixels + their fcTL dicts -> (F, H, W, 4): the canvas after each frame, before its dispose_op"""
    canvas = np.zeros((H, W, 4), np.uint8)
    out = np.zeros((len(frames), H, W, 4), np.uint8)
    for k, (px, fr) in enumerate(zip(pixels, frames)):
        x, y, w, h, dop = fr["x"], fr["y"], fr["width"], fr["height"], fr["dispose"]
        if k == 0 and dop == PREVIOUS:
            dop = BACKGROUND
        reg = canvas[y: y + h, x: x + w]
        saved = reg.copy() if dop == PREVIOUS else None
        reg[...] = px if fr["blend"] == SOURCE else over(px, reg)
        out[k] = canvas
        if dop == BACKGROUND:
            reg[...] = 0
        elif dop == PREVIOUS:
            reg[...] = saved
    return out


def decode(data, out_cap=None):
    """-> (status, frames (F, H, W, 4) uint8 or None, info: the png_info dict + num_frames, num_plays,
    default_is_frame, frames)"""
    data = bytes(data)
    st, inf, rest = R._walk(data)
    info = dict(inf, num_frames=0, num_plays=0, default_is_frame=0, frames=[])
    if st != R.OK:
        return st, None, info
    _, _, chunks, _ = rest
    st, ai, streams = anim_walk(data, inf)
    info.update(ai)
    if st != R.OK:
        return st, None, info
    for z in streams:
        if len(z) < 2 or (z[0] & 15) != 8 or (z[0] >> 4) > 7 or ((z[0] << 8) | z[1]) % 31 or (z[1] & 0x20):
            return R.E_ZLIB, None, info
    W, H = inf["width"], inf["height"]
    if out_cap is not None and out_cap < len(streams) * W * H * 4:
        return R.E_OUTPUT, None, info
    import zlib

    for body, crc in chunks:
        if zlib.crc32(body) & 0xFFFFFFFF != crc:
            return R.E_CRC, None, info
    head = []
    for t, b in _chunks(data):
        if t == b"IDAT":
            break
        if t in (b"PLTE", b"tRNS"):
            head.append((t, b))
    results = []
    for fr, z in zip(info["frames"], streams):
        ihdr = struct.pack(">IIBBBBB", fr["width"], fr["height"], inf["bit_depth"], inf["color_type"], 0, 0, inf["interlace"])
        png = R.SIG + R.chunk(b"IHDR", ihdr) + b"".join(R.chunk(t, b) for t, b in head) + R.chunk(b"IDAT", z) + \
            R.chunk(b"IEND", b"")
        results.append(R.decode(png))
    for group in ((R.E_INFLATE, R.E_DATA_LONG, R.E_DATA_SHORT), (R.E_ADLER,), (R.E_FILTER,), (R.E_PALETTE,)):
        for s, _, _ in results:
            if s in group:
                return s, None, info
    assert all(s == R.OK for s, _, _ in results)
    return R.OK, composite([px for _, px, _ in results], info["frames"], W, H), info
