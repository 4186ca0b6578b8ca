"""TEST HELPER: damaged PNG files for the differential tests of the PNG calls (include/decode_png.h), and what each of them
must come back as.  numpy + the stdlib's zlib + tests/png_spec_ref.py only; everything is deterministic from a seed.

  * base_files()        -- one small valid file per de-filter route and sample unit (stored, fixed and dynamic blocks, IDAT
                           split into several chunks, one of them empty);
  * corpus()            -- [Case]: the families C (container), H (IHDR rewrites), K (one flipped bit per chunk), P (damage
                           under a valid compression), T (zlib header and trailer), Z (damage in the DEFLATE data);
  * huge_ihdr_cases()   -- IHDR sizes up to 2^31 for the raw C call with small out_caps;
  * expectation(...)    -- the two-armed expectation: tests/png_spec_ref.py is authoritative everywhere except for files
                           whose DEFLATE data zlib rejects; there the CPU oracle of the shared inflate decides, and where
                           its size gates or its undefined-behaviour flags rule it out only the set of late statuses is
                           known (weak arm);
  * apng_corpus()       -- the container sweep for two small APNG files (host-only walk);
  * python tests/png_damage.py --host-corpus FILE  writes the host-decided cases for tools/asan_png_walk.c.
"""
import collections
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_spec_ref as R  # noqa: E402

Case = collections.namedtuple("Case", "family name data")
Expect = collections.namedtuple("Expect", "arm allowed pixels host ref_status")
LATE = frozenset((R.E_INFLATE, R.E_DATA_SHORT, R.E_DATA_LONG, R.E_ADLER))
FAMILIES = "CHKPTZ"
ORC_UB_OVERSUBSCRIBED = 0x10  # oracle/debig_oracle.h


# ------------------------------------------------------------------------------------------------ base files
def deflate(raw, mode):
    """raw -> (RFC 1951 data, byte offset of the final block's header: BFINAL is bit 0 of that byte).
    mode: 'stored' | 'fixed' | 'dynamic' | 'mixed' (a stored block, an empty stored block, then a compressed block)"""
    if mode == "stored":
        c = zlib.compressobj(0, zlib.DEFLATED, -15)
        return c.compress(raw) + c.flush(), 0
    if mode == "fixed":
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
        return c.compress(raw) + c.flush(), 0
    if mode == "dynamic":
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        return c.compress(raw) + c.flush(), 0
    assert mode == "mixed"
    k = min(24, len(raw) // 4)
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    a = c.compress(raw[:k]) + c.flush(zlib.Z_FULL_FLUSH)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return a + c.compress(raw[k:]) + c.flush(), len(a)


def zwrap(raw, mode):
    """-> (zlib stream, offset of the final block's header inside it)"""
    d, fin = deflate(raw, mode)
    return b"\x78\x9c" + d + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF), 2 + fin


def _content(rng, w, h, ct, depth, n_pal):
    """smooth, compressible raw samples with a little noise"""
    y, x = np.mgrid[0:h, 0:w]
    ch = R.CHANNELS[ct]
    if ct == 3:
        return ((x // 3 + y // 2) % n_pal).astype(np.uint8)[:, :, None]
    if depth < 8:
        return ((x // 5 + y // 3) % (1 << depth)).astype(np.uint8)[:, :, None]
    base = (x * 3 + y * 5)[:, :, None] + np.arange(ch) * 7
    noise = (rng.integers(0, 16, size=(h, w, ch)) == 0).astype(np.int64)
    if depth == 16:
        return ((base * 257 + noise * 3) % 65536).astype(np.uint16)
    return ((base // 2 + noise) % 256).astype(np.uint8)


# name, colour type, depth, interlace, w, h, block mode, sizes of the first IDAT chunks (the rest goes into the last one)
_BASES = (("rgba8", 6, 8, 0, 9, 70, "dynamic", (1, 0, 40)),      # tuned de-filter, crosses a 64-row band
          ("rgb8", 2, 8, 0, 31, 17, "fixed", (0, 33)),           # tuned de-filter
          ("rgb8key", 2, 8, 0, 13, 11, "stored", (3, 0)),        # tRNS key: general kernel; scan < z_total on purpose
          ("pal4il", 3, 4, 1, 37, 29, "mixed", (50, 0)),         # PLTE + tRNS + ancillary chunks, Adam7, sub-byte
          ("g16il", 0, 16, 1, 19, 14, "dynamic", (0, 20)),
          ("g1", 0, 1, 0, 70, 33, "fixed", (10, 0)),
          ("ga8", 4, 8, 0, 12, 9, "mixed", (0,)),
          ("rgba16", 6, 16, 0, 7, 8, "fixed", (5, 0, 5)))
N_PAL = 11


class Base:
    """one valid file: .data, and what it was made from"""

    def __init__(self, rng, name, ct, depth, il, w, h, mode, split):
        self.name, self.ct, self.depth, self.il, self.w, self.h, self.mode, self.split = name, ct, depth, il, w, h, mode, split
        self.samples = _content(rng, w, h, ct, depth, N_PAL)
        self.head = []  # chunks between IHDR and the first IDAT
        self.tail = []  # chunks between the last IDAT and IEND
        self.n_pal = 0
        if name == "rgb8key":
            self.head.append((b"tRNS", np.asarray(self.samples[2, 3], dtype=">u2").tobytes()))
        if ct == 3:
            self.n_pal = N_PAL
            pal = rng.integers(0, 256, size=(N_PAL, 3), dtype=np.uint8)
            self.head += [(b"gAMA", struct.pack(">I", 45455)), (b"PLTE", pal.tobytes()),
                          (b"tRNS", bytes(rng.integers(0, 256, size=7, dtype=np.uint8))), (b"tEXt", b"Title\0damage")]
            self.tail.append((b"tEXt", b"Comment\0after the data"))
        self.ihdr = struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, il)
        self.raw = R.scanlines(self.samples, ct, depth, il)
        self.z, self.fin = zwrap(self.raw, mode)
        self.scan = R.scanline_size(w, h, ct, depth, il)
        assert self.scan == len(self.raw)
        self.data = self.file()

    def chunks(self, z=None, ihdr=None):
        """[(type, body)] of the file with this zlib stream / IHDR body"""
        z = self.z if z is None else z
        pieces, rest = [], z
        for s in self.split:
            pieces.append(rest[:s])
            rest = rest[s:]
        pieces.append(rest)
        return [(b"IHDR", self.ihdr if ihdr is None else ihdr)] + self.head + [(b"IDAT", p) for p in pieces] + self.tail + \
            [(b"IEND", b"")]

    def file(self, z=None, ihdr=None):
        return assemble(self.chunks(z, ihdr))

    def file_of_raw(self, raw, mode=None):
        """the file around another scanline stream, validly compressed (fresh Adler-32)"""
        return self.file(zwrap(bytes(raw), mode or self.mode)[0])

    def row_offsets(self):
        """[(pass, row, offset of the filter byte in the scanline stream, row bytes)]"""
        out, pos = [], 0
        for p, (_, _, _, _, wp, hp) in enumerate(R.passes(self.w, self.h, self.il)):
            rb = R.row_bytes(wp, self.ct, self.depth)
            for y in range(hp):
                out.append((p, y, pos, rb))
                pos += 1 + rb
        return out


def assemble(chunks):
    return R.SIG + b"".join(R.chunk(t, b) for t, b in chunks)


def spans(data):
    """[(offset of the length field, body length, type)] of a VALID file's chunks"""
    out, pos = [], 8
    while pos < len(data):
        ln = struct.unpack(">I", data[pos: pos + 4])[0]
        out.append((pos, ln, data[pos + 4: pos + 8]))
        pos += 12 + ln
    return out


_CACHE = {}
_EXPECT = {}


def expectations(cases, oracle):
    """[Expect] for the cases, computed once per file (and per kind of caller: with or without an oracle) and kept"""
    out = []
    for c in cases:
        key = (c.name, c.data, oracle is None)
        if key not in _EXPECT:
            _EXPECT[key] = expectation(c, oracle)
        out.append(_EXPECT[key])
    return out


def base_files(seed=1):
    if seed not in _CACHE:
        rng = np.random.default_rng(seed)
        _CACHE[seed] = [Base(rng, *b) for b in _BASES]
    return _CACHE[seed]


# ------------------------------------------------------------------------------------------------ the families
def _put(data, off, b):
    return data[:off] + b + data[off + len(b):]


def _flip(data, off, mask):
    return data[:off] + bytes([data[off] ^ mask]) + data[off + 1:]


def _container(b):
    d = b.data
    for k in range(len(d)):
        yield "prefix %d" % k, d[:k]
    sp = spans(d)
    for off, ln, typ in sp:
        t = typ.decode()
        end = len(d) - (off + 12)
        vals = [0, 1, ln - 1, ln + 1, ln + 4, ln + 12, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, end, end + 1]
        for v in sorted(set(v for v in vals if 0 <= v <= 0xFFFFFFFF and v != ln)):
            yield "%s@%d length %d" % (t, off, v), _put(d, off, struct.pack(">I", v))
        for k in range(4):
            for mask in (0x20, 0x01, 0x80):
                yield "%s@%d type byte %d ^ %#x" % (t, off, k, mask), _flip(d, off + 4 + k, mask)
    pieces = [d[off: off + 12 + ln] for off, ln, _ in sp]
    for i, (off, ln, typ) in enumerate(sp):
        t = typ.decode()
        yield "%s@%d dropped" % (t, off), d[:8] + b"".join(pieces[:i] + pieces[i + 1:])
        yield "%s@%d doubled" % (t, off), d[:8] + b"".join(pieces[:i + 1] + pieces[i:])
        if i + 1 < len(sp):
            yield "%s@%d swapped" % (t, off), d[:8] + b"".join(pieces[:i] + [pieces[i + 1], pieces[i]] + pieces[i + 2:])
    yield "trailing byte", d + b"\0"
    yield "trailing text", d + b"junk" * 5
    yield "trailing chunks", d + d[8:]


def _ihdr(b):
    w, h = b.w, b.h
    rewrites = []
    for ct in range(8):
        for depth in (0, 1, 2, 3, 4, 8, 16, 32):
            if (ct, depth) != (b.ct, b.depth):
                rewrites.append(("pair %d/%d" % (ct, depth), struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, b.il)))
    for il in (0, 1, 2):
        if il != b.il:
            rewrites.append(("interlace %d" % il, struct.pack(">IIBBBBB", w, h, b.depth, b.ct, 0, 0, il)))
    for comp, filt in ((1, 0), (0, 1), (255, 0), (0, 255)):
        rewrites.append(("compression %d filter %d" % (comp, filt), struct.pack(">IIBBBBB", w, h, b.depth, b.ct, comp, filt, b.il)))
    for nw, nh in ((w + 1, h), (w - 1, h), (w * 2, h), (w // 2, h), (1, h), (w, h + 1), (w, h - 1), (w, h * 2), (w, h // 2),
                   (w, 1), (1, 1), (0, h), (w, 0)):
        rewrites.append(("size %dx%d" % (nw, nh), struct.pack(">IIBBBBB", nw, nh, b.depth, b.ct, 0, 0, b.il)))
    for name, body in rewrites:
        yield name, b.file(ihdr=body)
        yield name + ", CRC kept", _put(b.data, 16, body)  # IHDR's body lies at 16; its CRC stays that of the old body
    yield "IHDR 12 bytes", assemble([(b"IHDR", b.ihdr[:12])] + b.chunks()[1:])
    yield "IHDR 14 bytes", assemble([(b"IHDR", b.ihdr + b"\0")] + b.chunks()[1:])


def huge_ihdr_cases():
    """(name, file, out_cap): sizes the Python wrappers cannot take -- the raw C call, small out_caps"""
    b = base_files()[0]
    out = []
    for w, h in ((0x7FFFFFFF, 1), (1, 0x7FFFFFFF), (0x7FFFFFFF, 0x7FFFFFFF), (0x80000000, 1), (1, 0x80000000), (0x80000000, 0x80000000),
                 (0xFFFFFFFF, 7), (65536, 65536), (0x7FFFFFFF, b.h), (b.w, 0x7FFFFFFF)):
        for cap in (0, 64, 4 * b.w * b.h):
            out.append(("huge %#x x %#x cap %d" % (w, h, cap), b.file(ihdr=struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)), cap))
    return out


def _bitflips(b):
    d = b.data
    for i, (off, ln, typ) in enumerate(spans(d)):
        t = typ.decode()
        yield "%s@%d CRC bit" % (t, off), _flip(d, off + 8 + ln + (i % 4), 1 << (i % 8))
        yield "%s@%d type bit" % (t, off), _flip(d, off + 4 + (i % 4), 0x02 << (i % 3))
        if ln:
            yield "%s@%d body bit (middle)" % (t, off), _flip(d, off + 8 + ln // 2, 1 << ((i + 3) % 8))
            # (IHDR: the low byte of the width, so that the image stays small enough for every wrapper to allocate)
            yield "%s@%d body bit (first)" % (t, off), _flip(d, off + 8 + (3 if typ == b"IHDR" else 0), 0x40)
            yield "%s@%d body bit (last)" % (t, off), _flip(d, off + 8 + ln - 1, 0x01)


def _under_valid_compression(b):
    rows = b.row_offsets()
    raw = bytearray(b.raw)
    n_pass = rows[-1][0]
    picks = {"first row": rows[0], "middle row": rows[len(rows) // 2], "last row": rows[-1]}
    if b.il:
        picks["first row of the last pass"] = [r for r in rows if r[0] == n_pass][0]
        picks["last row of the first pass"] = [r for r in rows if r[0] == 0][-1]
    if not b.il and b.h > 65:
        picks["row 63"] = rows[63]
        picks["row 64"] = rows[64]
    for name, (_, _, pos, _) in picks.items():
        for v in (5, 255):
            r = bytearray(raw)
            r[pos] = v
            yield "filter %d in the %s" % (v, name), b.file_of_raw(r)
    if b.ct == 3:
        per = 8 // b.depth
        ylast = [y for y in range(b.h)][b.h // 2]
        bad = {"first pixel": (0, 0), "last pixel": (b.h - 1, b.w - 1), "last sample of a row": (ylast, b.w - 1)}
        assert b.w % per, "the last byte of a row must be partly filled"
        for name, (y, x) in bad.items():
            for v in (b.n_pal, (1 << b.depth) - 1):
                s = b.samples.copy()
                s[y, x, 0] = v
                yield "palette index %d at the %s" % (v, name), b.file_of_raw(R.scanlines(s, b.ct, b.depth, b.il))
        s = b.samples.copy()
        s[0, 0, 0] = b.n_pal
        r = bytearray(R.scanlines(s, b.ct, b.depth, b.il))
        r[rows[-1][2]] = 7
        yield "palette index and filter type together", b.file_of_raw(r)
    rb = rows[-1][3] + 1
    yield "scanlines 1 byte short", b.file_of_raw(raw[:-1])
    yield "scanlines a row short", b.file_of_raw(raw[:-rb])
    yield "scanlines 1 byte long", b.file_of_raw(raw + b"\0")
    yield "scanlines a row long", b.file_of_raw(raw + raw[-rb:])
    yield "scanlines 300 bytes long", b.file_of_raw(raw + bytes(range(256)) + bytes(44))
    yield "scanlines 70000 bytes long", b.file_of_raw(raw + bytes(70000), "dynamic" if b.mode == "stored" else None)
    if len(raw) > 300:
        yield "scanlines 300 bytes short", b.file_of_raw(raw[:-300])
    yield "no scanlines", b.file_of_raw(b"")


def _fcheck(cmf, flg):
    return bytes([cmf, (flg & 0xE0) | ((31 - ((cmf << 8) | (flg & 0xE0)) % 31) % 31)])


def _trailer_and_header(b):
    z = b.z
    for k in range(4):
        yield "Adler-32 byte %d" % k, b.file(_flip(z, len(z) - 4 + k, 0x80 >> k))
    for k in (3, 2, 1, 0):
        yield "trailer cut to %d bytes" % k, b.file(z[: len(z) - 4 + k])
    yield "trailer of zeros", b.file(z[:-4] + bytes(4))
    yield "bytes after the trailer", b.file(z + b"\1\2\3\4\5")
    ch = b.chunks()
    last = max(i for i, (t, _) in enumerate(ch) if t == b"IDAT")
    body = ch[last][1]
    for cut in (4, 2, 1):
        if len(body) > cut:
            moved = ch[:last] + [(b"IDAT", body[:-cut]), (b"IDAT", body[-cut:])] + ch[last + 1:]
            yield "last %d trailer bytes in an IDAT chunk of their own" % cut, assemble(moved)
    for cm in (0, 7, 9, 15):
        yield "zlib CM %d" % cm, b.file(_fcheck(0x70 | cm, z[1]) + z[2:])
    for cinfo in range(16):
        if cinfo != 7:
            yield "zlib CINFO %d" % cinfo, b.file(_fcheck((cinfo << 4) | 8, z[1]) + z[2:])
    for mask in (0x01, 0x10, 0x1F):
        yield "zlib FCHECK ^ %#x" % mask, b.file(bytes([z[0], z[1] ^ mask]) + z[2:])
    yield "zlib FDICT", b.file(_fcheck(z[0], z[1] | 0x20) + z[2:])
    yield "zlib FDICT with a dictionary id", b.file(_fcheck(z[0], z[1] | 0x20) + b"\0\0\0\1" + z[2:])
    for lvl in (0, 1, 3):
        yield "zlib FLEVEL %d" % lvl, b.file(_fcheck(z[0], lvl << 6) + z[2:])
    yield "zlib header only", b.file(z[:2])
    yield "zlib 1 byte", b.file(z[:1])
    yield "zlib empty", b.file(b"")


# files whose every DEFLATE byte is flipped once: one per block type (mixed: stored + compressed)
_DENSE = ("rgba8", "rgb8", "pal4il", "rgb8key")


def _deflate_damage(b, rng):
    z = b.z
    stride = 1 if b.name in _DENSE else 5
    for i in range(2, len(z) - 4, stride):
        bit = int(rng.integers(0, 8))
        yield "bit %d of byte %d" % (bit, i), b.file(_flip(z, i, 1 << bit))
    for k in sorted(set(int(v) for v in np.linspace(2, len(z) - 1, 40))):
        yield "truncated to %d bytes" % k, b.file(z[:k])
    yield "BFINAL cleared", b.file(_flip(z, b.fin, 1))
    yield "BFINAL cleared, trailer cut", b.file(_flip(z, b.fin, 1)[:-4])


def corpus(seed=1, families=FAMILIES):
    """every damaged file of the chosen families, [Case(family, name, data)]; names are unique"""
    out = []
    rng = np.random.default_rng(seed + 1000)
    gens = {"C": _container, "H": _ihdr, "K": _bitflips, "P": _under_valid_compression, "T": _trailer_and_header}
    for b in base_files(seed):
        for fam in families:
            it = _deflate_damage(b, rng) if fam == "Z" else gens[fam](b)
            for name, data in it:
                out.append(Case(fam, "%s %s: %s" % (fam, b.name, name), bytes(data)))
    return out


def thin(cases, per_family, seed=7):
    """a deterministic subset: at most per_family cases of every family (a dict, or one number for all)"""
    rng = np.random.default_rng(seed)
    out = []
    for fam in FAMILIES:
        sub = [c for c in cases if c.family == fam]
        cap = per_family[fam] if isinstance(per_family, dict) else per_family
        if len(sub) > cap:
            keep = sorted(rng.choice(len(sub), size=cap, replace=False))
            sub = [sub[i] for i in keep]
        out += sub
    return out


# ------------------------------------------------------------------------------------------------ the expectation
def expectation(case, oracle=None):
    """what every PNG call must answer for this file -> Expect(arm, allowed statuses, pixels or None, host, ref_status)
    arm 'exact':  tests/png_spec_ref.py decides status and pixels;
    arm 'oracle': a file whose DEFLATE data zlib rejects, decided by the CPU oracle of the shared inflate;
    arm 'weak':   such a file outside the oracle's domain: one of the four late statuses, never OK;
    arm 'oversubscribed': a file of the weak arm whose only oracle flag is an over-subscribed code-length set: E_INFLATE.
    host: the status is decided without the device (the chunk walk, or the zlib header)."""
    data = case.data
    wst, inf, rest = R._walk(data)
    st, px, _ = R.decode(data)
    host = wst != R.OK or st == R.E_ZLIB
    if st != R.E_INFLATE:
        return Expect("exact", frozenset((st,)), px, host, st)
    # zlib rejects the DEFLATE data.  (Z cases by construction; of the other families only the few files whose IDAT
    # concatenation is cut short or spliced -- an IDAT chunk dropped or doubled, a zlib header with nothing behind it.)
    pal, key, _, z = rest
    scan = R.scanline_size(inf["width"], inf["height"], inf["color_type"], inf["bit_depth"], inf["interlace"])
    if oracle is None or not (len(z) - 2 >= 5 and scan >= len(z) - 2):
        return Expect("weak", LATE, None, False, st)
    good, final, produced, stats = oracle.inflate(z[2:], scan, want_stats=True)
    full = None  # what the pixels step gives if the oracle's output is complete and passes the file's own Adler-32
    if good and final == scan:
        t = 2 + (stats.bits_consumed + 7) // 8
        if t + 4 <= len(z) and struct.unpack(">I", z[t: t + 4])[0] == zlib.adler32(produced) & 0xFFFFFFFF:
            full = R.pixels(produced, inf, pal, key)
    if stats.ub_flags == ORC_UB_OVERSUBSCRIBED:
        # an over-subscribed code-length set and nothing else: the oracle (like the reference) decodes on, the kernels fail
        # a stream with DEBIG_STREAM_NO_REF_GATES at that block's header (include/debig_hip.h), at every width alike
        return Expect("oversubscribed", frozenset((R.E_INFLATE,)), None, False, st)
    if stats.ub_flags != 0 or (good and final is None):
        return Expect("weak", LATE, None, False, st)
    if not good:
        return Expect("oracle", frozenset((R.E_INFLATE, R.E_DATA_LONG)), None, False, st)
    if final < scan:
        return Expect("oracle", frozenset((R.E_DATA_SHORT,)), None, False, st)
    if full is None:
        return Expect("oracle", frozenset((R.E_ADLER,)), None, False, st)
    return Expect("oracle", frozenset((full[0],)), full[1], False, st)


def stream_of(data):
    """(IDAT concatenation, scanline size, info, palette, key) of a file whose walk passes"""
    wst, inf, rest = R._walk(data)
    assert wst == R.OK
    pal, key, _, z = rest
    return z, R.scanline_size(inf["width"], inf["height"], inf["color_type"], inf["bit_depth"], inf["interlace"]), inf, pal, key


# ------------------------------------------------------------------------------------------------ APNG
def apng_bases(seed=1):
    """two small APNG files as chunk lists [(type, body)]"""
    import apng_ref as A

    rng = np.random.default_rng(seed + 50)
    f0 = [A.frame(_content(rng, 9, 7, 6, 8, 0)), A.frame(_content(rng, 4, 3, 6, 8, 0), x=5, y=4, dispose=A.BACKGROUND, blend=A.OVER),
          A.frame(_content(rng, 9, 7, 6, 8, 0), dispose=A.PREVIOUS)]
    a = A.apng_chunks(f0, 6, 8, fdat_split=[7])
    pal = [(i * 20, 255 - i * 20, i) for i in range(N_PAL)]
    f1 = [A.frame(_content(rng, 5, 6, 3, 4, N_PAL), x=1, y=2), A.frame(_content(rng, 8, 8, 3, 4, N_PAL), blend=A.OVER)]
    b = A.apng_chunks(f1, 3, 4, interlace=1, palette=pal, trns=b"\0\x80", default=_content(rng, 8, 8, 3, 4, N_PAL))
    return [("apng rgba8", a), ("apng pal4 default", b)]


def apng_corpus(seed=1):
    """[(name, file)]: prefixes, chunk drop / dup / swap, sequence numbers +-1, regions one pixel outside the canvas,
    acTL's frame count +-1"""
    import apng_ref as A

    out = []
    for bname, ch in apng_bases(seed):
        d = A.assemble(ch)
        W, H = struct.unpack(">II", ch[0][1][:8])
        out.append((bname + ": undamaged", d))
        for k in range(len(d)):
            out.append(("%s: prefix %d" % (bname, k), d[:k]))
        for i, (t, body) in enumerate(ch):
            n = "%s: %s #%d " % (bname, t.decode(), i)
            out.append((n + "dropped", A.assemble(ch[:i] + ch[i + 1:])))
            out.append((n + "doubled", A.assemble(ch[:i + 1] + ch[i:])))
            if i + 1 < len(ch):
                out.append((n + "swapped", A.assemble(ch[:i] + [ch[i + 1], ch[i]] + ch[i + 2:])))
            if t in (b"fcTL", b"fdAT"):
                seq = struct.unpack(">I", body[:4])[0]
                for v in (seq + 1, seq - 1):
                    if v >= 0:
                        out.append((n + "sequence %d" % v, A.assemble(ch[:i] + [(t, struct.pack(">I", v) + body[4:])] + ch[i + 1:])))
                out.append((n + "renumbered after a drop", A.assemble(A.renumber(ch[:i] + ch[i + 1:]))))
            if t == b"fcTL":
                s, w, h, x, y = struct.unpack(">IIIII", body[:20])
                for nw, nh, nx, ny in ((W - x + 1, h, x, y), (w, H - y + 1, x, y), (w, h, W - w + 1, y), (w, h, x, H - h + 1),
                                       (0, h, x, y), (w, 0, x, y), (w, h, 0xFFFFFFFF, y), (0xFFFFFFFF, h, 1, y)):
                    nb = struct.pack(">IIIII", s, nw, nh, nx, ny) + body[20:]
                    out.append((n + "region %dx%d at %d,%d" % (nw, nh, nx, ny), A.assemble(ch[:i] + [(t, nb)] + ch[i + 1:])))
                for dop, bop in ((3, 0), (0, 2)):
                    out.append((n + "dispose %d blend %d" % (dop, bop), A.assemble(ch[:i] + [(t, body[:24] + bytes([dop, bop]))] + ch[i + 1:])))
                out.append((n + "25 bytes", A.assemble(ch[:i] + [(t, body[:25])] + ch[i + 1:])))
            if t == b"acTL":
                nf = struct.unpack(">I", body[:4])[0]
                for v in (nf + 1, nf - 1, 0):
                    out.append((n + "frame count %d" % v, A.assemble(ch[:i] + [(t, struct.pack(">I", v) + body[4:])] + ch[i + 1:])))
                out.append((n + "9 bytes", A.assemble(ch[:i] + [(t, body + b"\0")] + ch[i + 1:])))
    return out


def apng_walk_ref(data):
    """the status of the host-only walk (debig_apng_info_get): the chunk walk, then the animation rules -> (status, info)"""
    import apng_ref as A

    data = bytes(data)
    st, inf, _ = R._walk(data)
    info = dict(inf, num_frames=0, num_plays=0, default_is_frame=0, frames=[])
    if st != R.OK:
        return st, info
    st, ai, _ = A.anim_walk(data, inf)
    info.update(ai)
    return st, info


# ------------------------------------------------------------------------------------------------ corpus file
def write_host_corpus(path, seed=1):
    """the host-decided C / H / T cases, the huge IHDR sizes and the APNG sweep for tools/asan_png_walk.c.  Records, all
    little-endian: u32 kind (0 PNG, 1 APNG walk only), u32 status of debig_png_decode_batch, u32 status of
    debig_png_info_get, u32 status of debig_apng_info_get, u64 out_cap, u32 length, the file."""
    n = 0
    with open(path, "wb") as f:
        def rec(kind, st, ist, ast, cap, data):
            f.write(struct.pack("<IIIIQI", kind, st, ist, ast, cap, len(data)) + data)

        for c in corpus(seed, "CHT"):
            e = expectation(c)
            if not e.host:
                continue
            rec(0, e.ref_status, R.info(c.data)[0], apng_walk_ref(c.data)[0], 1 << 20, c.data)
            n += 1
        for _, data, cap in huge_ihdr_cases():
            rec(0, R.decode(data, out_cap=cap)[0], R.info(data)[0], apng_walk_ref(data)[0], cap, data)
            n += 1
        for _, data in apng_corpus(seed):
            rec(1, 0, 0, apng_walk_ref(data)[0], 0, data)
            n += 1
    return n


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--host-corpus":
        print("%d records" % write_host_corpus(sys.argv[2]))
    else:
        sys.exit("usage: python tests/png_damage.py --host-corpus FILE")
