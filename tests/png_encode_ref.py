"""TEST TOOLING: a numpy restatement of the PNG encode (include/decode_png.h: debig_png_encode_batch; csrc/png_encode_kernel.inc):
the filtered scanline stream for every filter mode (ADAPTIVE: the minimum sum of min(b, 256 - b), ties to the lowest type), the
container, the bound, the chunk cut, check_task() -- what one deflate task's output must be, judged by zlib -- and a small bit
reader that lists a task's blocks.  Nothing here looks at the kernels' code."""
import struct
import zlib

import numpy as np

from png_spec_ref import SIG, chunk
import png_spec_ref as S

CHUNK = 32768  # include/debig_hip.h: DEBIG_PNG_ENCODE_CHUNK
FILTER_BYTES = 65536  # DEBIG_PNG_ENCODE_FILTER_BYTES
NO_STORED = 1  # DEBIG_PNG_ENCODE_NO_STORED
FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
E_OUTPUT, E_ENCODE, E_RANGE, BAD_ARG = 12, 20, 21, -2
COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}


def slot_bytes(n):
    """DEBIG_PNG_ENCODE_SLOT"""
    return (n + n // 8 + 32 + 15) // 16 * 16


def raw_rows(img, depth):
    """(H, W, C) sample values -> (H, row_bytes) uint8, 16-bit samples big-endian"""
    img = np.asarray(img)
    H = img.shape[0]
    if depth == 16:
        return img.astype(">u2").reshape(H, -1).view(np.uint8).reshape(H, -1)
    return img.astype(np.uint8).reshape(H, -1)


def filtered_rows(raw, bpp):
    """(H, rb) raw bytes -> (5, H, rb): the rows under each filter type"""
    raw = raw.astype(np.int32)
    H, rb = raw.shape
    a = np.zeros_like(raw)
    a[:, bpp:] = raw[:, : max(rb - bpp, 0)]
    b = np.zeros_like(raw)
    b[1:] = raw[:-1]
    c = np.zeros_like(raw)
    c[1:, bpp:] = raw[:-1, : max(rb - bpp, 0)]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([raw, raw - a, raw - b, raw - ((a + b) >> 1), raw - paeth]) & 255


def filter_types(raw, bpp, filt):
    """the filter type of every row"""
    H = raw.shape[0]
    if filt != 5:
        return np.full(H, filt, np.int64)
    f = filtered_rows(raw, bpp)
    cost = np.minimum(f, 256 - f).sum(axis=2)  # (5, H)
    return np.argmin(cost, axis=0)  # the first minimum: ties to the lowest type


def filtered_stream(img, depth, filt):
    """img (H, W, C) -> the bytes the file's zlib stream inflates to"""
    img = np.asarray(img)
    H, W, Cn = img.shape
    bpp = Cn * depth // 8
    raw = raw_rows(img, depth)
    f = filtered_rows(raw, bpp)
    types = filter_types(raw, bpp, filt)
    out = np.zeros((H, 1 + raw.shape[1]), np.uint8)
    out[:, 0] = types
    out[:, 1:] = f[types, np.arange(H)]
    return out.tobytes()


def chunks(n):
    """[(offset, length)] of a stream of n bytes"""
    return [(o, min(CHUNK, n - o)) for o in range(0, n, CHUNK)]


def row_runs(H, rb):
    """the rows of one filter task as the host cuts them"""
    per = 1 if rb >= FILTER_BYTES else FILTER_BYTES // rb
    return [(y, min(per, H - y)) for y in range(0, H, per)]


def head(W, H, Cn, depth, palette=None, trns=None):
    """the file up to the IDAT chunk"""
    ct = 3 if palette is not None else COLOR_TYPE[Cn]
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ct, 0, 0, 0))
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None and len(trns):
        out += chunk(b"tRNS", bytes(bytearray(trns)))
    return out


def container(W, H, Cn, depth, zdata, palette=None, trns=None):
    return head(W, H, Cn, depth, palette, trns) + chunk(b"IDAT", zdata) + chunk(b"IEND", b"")


def stored_payload(n):
    """the DEFLATE bytes of a stream of n bytes at level 0: 5 + len per chunk, 5 more behind every chunk but the last"""
    return sum(5 + ln for _, ln in chunks(n)) + 5 * (len(chunks(n)) - 1)


def bound(W, H, Cn, depth, pal=0, trns=0):
    """debig_png_encode_bound: the level-0 file (level 1 is never longer)"""
    n = H * (1 + W * Cn * depth // 8)
    return 8 + 25 + (12 + 3 * pal if pal else 0) + (12 + trns if trns else 0) + 12 + 2 + stored_payload(n) + 4 + 12


def check_task(output, k, stream):
    """the bytes of deflate task k of `stream`, alone: complete blocks that hold exactly the chunk"""
    cuts = chunks(len(stream))
    off, ln = cuts[k]
    last = k == len(cuts) - 1
    d = zlib.decompressobj(-15, zdict=stream[max(0, off - 32768): off]) if off else zlib.decompressobj(-15)
    got = d.decompress(bytes(output))
    assert got == stream[off: off + ln], (k, len(got), ln)
    assert d.eof == last, (k, d.eof, last)
    assert d.unused_data == b"", (k, len(d.unused_data))
    if not last:
        assert bytes(output[-4:]) == b"\x00\x00\xff\xff", (k, bytes(output[-8:]))


class _Bits:
    def __init__(self, data):
        self.d = bytes(data)
        self.n = 8 * len(self.d)
        self.at = 0

    def take(self, k):
        assert self.at + k <= self.n, "the blocks run past the task's bytes"
        lo = self.at >> 3
        r = (int.from_bytes(self.d[lo: lo + 5], "little") >> (self.at & 7)) & ((1 << k) - 1)  # k <= 16
        self.at += k
        return r

    def skip(self, k):
        assert self.at + k <= self.n, "the blocks run past the task's bytes"
        self.at += k

    def code(self, k):
        """k bits, most significant first"""
        r = 0
        for _ in range(k):
            r = (r << 1) | self.take(1)
        return r


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
          16385, 24577]
_DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def blocks(data):
    """the DEFLATE blocks in `data` (stored and fixed-Huffman only) ->
    [{"final", "btype", "bytes": what the block holds, "matches": [(length, distance)], "end": the bit behind it}]"""
    b = _Bits(data)
    out = []
    while b.n - b.at >= 3 and not (out and out[-1]["final"]):
        final, btype = b.take(1), b.take(2)
        assert btype in (0, 1), ("a block type that the encoder never writes", btype)
        blk = {"final": final, "btype": btype, "bytes": 0, "matches": []}
        if btype == 0:
            b.at = (b.at + 7) & ~7
            ln, nln = b.take(16), b.take(16)
            assert ln == (~nln & 0xFFFF)
            b.skip(8 * ln)
            blk["bytes"] = ln
        else:
            while True:
                c = b.code(7)
                if c <= 0b0010111:
                    sym = 256 + c
                else:
                    c = (c << 1) | b.take(1)
                    if 0b00110000 <= c <= 0b10111111:
                        sym = c - 0b00110000
                    elif 0b11000000 <= c <= 0b11000111:
                        sym = 280 + c - 0b11000000
                    else:
                        c = (c << 1) | b.take(1)
                        assert 0b110010000 <= c <= 0b111111111
                        sym = 144 + c - 0b110010000
                if sym == 256:
                    break
                if sym < 256:
                    blk["bytes"] += 1
                    continue
                assert sym <= 285
                ln = _LBASE[sym - 257] + b.take(_LEXT[sym - 257])
                dc = b.code(5)
                assert dc < 30
                dist = _DBASE[dc] + b.take(_DEXT[dc])
                assert 3 <= ln <= 258 and 1 <= dist <= 32768
                blk["bytes"] += ln
                blk["matches"].append((ln, dist))
        blk["end"] = b.at
        out.append(blk)
    # what is left behind the last block is the padding of its last byte
    assert b.n - b.at < 8 and (b.n == b.at or b.take(b.n - b.at) == 0), "bits behind the last block"
    return out


def samples_of(data):
    """a PNG file -> (status, (H, W, C) sample values at full depth (palette: indices), info, palette, trns key)"""
    st, inf, rest = S._walk(bytes(data))
    if st != S.OK:
        return st, None, inf, None, None
    pal, key, chunk_list, z = rest
    raw = zlib.decompress(z)
    w, h, ct, depth = inf["width"], inf["height"], inf["color_type"], inf["bit_depth"]
    rb = S.row_bytes(w, ct, depth)
    rows, bad, pos = S._unfilter(raw, 0, w, h, rb, S.bpp_f(ct, depth))
    assert bad is None and pos == len(raw)
    return st, S._samples(rows, w, ct, depth), inf, pal, key
