"""TEST TOOLING: the files of tests/test_gpu_gunzip.py (debig_gunzip_batch, include/decode_gz.h) with the status each must get, written
down by hand per case -- tests/test_gunzip_ref_cpu.py holds the restatement (tests/gunzip_ref.py) to these, and the GPU test holds the
library to the restatement.  Plain data: zlib writes the streams, struct the headers.  Members are 0 .. 20 000 bytes.

A Case is (name, file bytes or None for a NULL input entry, cap or None for a NULL output entry, expect).  expect is ONE status, or the
name of one of the two families whose answer is a set: CUT (a stream cut inside the DEFLATE data: E_TRUNCATED or E_INFLATE) and RACE
(an understated BGZF ISIZE: the next member writes over this one's last bytes while its CRC-32 is taken: E_CRC or E_ISIZE)."""
import collections
import random
import struct
import zlib

import gunzip_ref as R

Case = collections.namedtuple("Case", "name data cap expect")
CUT, RACE = "cut-stream", "isize-race"
FAMILY_SETS = {CUT: {R.E_TRUNCATED, R.E_INFLATE}, RACE: {R.E_CRC, R.E_ISIZE}}
SLACK = 64  # bytes of cap beyond the plain size where a case is not about the cap
BC = b"BC\x02\x00\x00\x00"


def blob(n, seed):
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(2, 9))) for _ in range(60)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + b" "
    return bytes(out[:n])


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def header(text=False, hcrc=False, extra=None, name=None, comment=None, mtime=0, xfl=0, os=255):
    flg = (1 if text else 0) | (2 if hcrc else 0) | (4 if extra is not None else 0) | (8 if name is not None else 0) | \
        (16 if comment is not None else 0)
    h = bytes([31, 139, 8, flg]) + struct.pack("<IBB", mtime, xfl, os)
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h


def trailer(data):
    return struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **fields):
    return header(**fields) + deflate(data, level, strategy) + trailer(data)


def bgzf(data, level=6, pre=b"", post=b"", bsize=None, delta=0):
    """a BGZF member: BC after the subfields `pre`, in front of `post`; BSIZE = its size - 1 + delta, or `bsize` as given"""
    m = bytearray(member(data, level, extra=pre + BC + post))
    struct.pack_into("<H", m, 12 + len(pre) + 4, len(m) - 1 + delta if bsize is None else bsize)
    return bytes(m)


EOF_BLOCK = bgzf(b"")
ALL_FIELDS = dict(text=True, hcrc=True, extra=b"XY\x03\x00abc", name=b"a name.txt", comment=b"a comment", mtime=0x5F3759DF, xfl=2, os=3)


LIE_PARTS = [blob(3000, 300), blob(2500, 301), blob(1, 302), blob(4000, 303)]  # the members of the lying BGZF files


def _patch(m, at, fmt, value):
    m = bytearray(m)
    struct.pack_into(fmt, m, at if at >= 0 else len(m) + at, value)
    return bytes(m)


def cases():
    out = []

    def add(name, data, expect, plain=b"", cap="fits"):
        out.append(Case(name, data, len(plain) + SLACK if cap == "fits" else cap, expect))

    # ---- headers
    d = blob(700, 1)
    for flg in range(32):
        f = dict(text=bool(flg & 1), hcrc=bool(flg & 2), extra=b"XY\x03\x00abc" if flg & 4 else None,
                 name=b"n%d" % flg if flg & 8 else None, comment=b"c%d" % flg if flg & 16 else None)
        add("hdr-flags-%02x" % flg, member(d, **f), R.OK, d)
    add("hdr-xlen-0", member(d, extra=b""), R.OK, d)
    add("hdr-empty-name", member(d, name=b""), R.OK, d)
    add("hdr-comment-300", member(d, comment=b"c" * 300), R.OK, d)
    add("hdr-mtime-xfl-os", member(d, mtime=0xFFFFFFFF, xfl=4, os=11), R.OK, d)
    h = header(**ALL_FIELDS)
    first = member(d, name=b"first")
    for cut in range(len(h) + 1):
        # alone: nothing of a header is E_TRUNCATED at every length; the whole header without a stream is a cut stream
        add("hdr-cut-%d-first" % cut, h[:cut], R.E_TRUNCATED if cut < len(h) else CUT)
        # behind a member: fewer than 10 bytes are trailing bytes, 10 and more are a header that runs out
        add("hdr-cut-%d-second" % cut, first + h[:cut],
            R.OK if cut == 0 else R.E_TRAILING if cut < 10 else R.E_TRUNCATED if cut < len(h) else CUT, d)
    good = member(d)
    for bit in (0x20, 0x40, 0x80):
        add("hdr-reserved-%02x" % bit, _patch(good, 3, "<B", bit), R.E_HEADER)
    add("hdr-cm-7", _patch(good, 2, "<B", 7), R.E_HEADER)
    add("hdr-magic-0", _patch(good, 0, "<B", 0x1E), R.E_HEADER)
    add("hdr-magic-1", _patch(good, 1, "<B", 0x8C), R.E_HEADER)
    add("hdr-reserved-second", first + _patch(good, 3, "<B", 0x80), R.E_HEADER, d)

    # ---- plain multi-member files: 1 .. 6 members, empty / stored / fixed / dynamic in turn
    kinds = [dict(level=6), dict(level=0), dict(level=6, strategy=zlib.Z_FIXED), dict(level=9), dict(level=1)]
    for n in range(1, 7):
        rng = random.Random(100 + n)
        parts = [b"" if (n + k) % 4 == 3 else blob(rng.randint(1, 20000), 110 + 10 * n + k) for k in range(n)]
        raw = b"".join(member(p, name=b"m%d" % k if k % 2 else None, **kinds[(n + k) % 5]) for k, p in enumerate(parts))
        add("plain-%d-members" % n, raw, R.OK, b"".join(parts))
    add("plain-only-empty-members", member(b"") + member(b"", level=0) + member(b"", strategy=zlib.Z_FIXED), R.OK)

    # ---- well-formed BGZF
    for n, size in ((1, 20000), (2, 20000), (300, 2000)):
        rng = random.Random(200 + n)
        parts = [blob(rng.randint(0, size), 210 + k) for k in range(n)]
        raw = b"".join(bgzf(p) for p in parts)
        add("bgzf-%d" % n, raw, R.OK, b"".join(parts))
        add("bgzf-%d-eof" % n, raw + EOF_BLOCK, R.OK, b"".join(parts))
    p3 = [blob(5000, 230), blob(1, 231), blob(12000, 232)]
    add("bgzf-bc-second-of-three", b"".join(bgzf(p, pre=b"XY\x01\x00a", post=b"ZZ\x00\x00") for p in p3), R.OK, b"".join(p3))
    add("bgzf-bc-slen-3-is-plain", b"".join(member(p, extra=b"BC\x03\x00\x07\x00\x00") for p in p3), R.OK, b"".join(p3))
    add("bgzf-xlen-cuts-last-subfield", b"".join(bgzf(p, post=b"QQ\x05\x00ab") for p in p3) + EOF_BLOCK, R.OK, b"".join(p3))
    add("bgzf-xlen-cuts-bc-is-plain", b"".join(member(p, extra=b"XY\x00\x00BC\x02\x00\x11") for p in p3), R.OK, b"".join(p3))
    add("bgzf-plain-bgzf", bgzf(p3[0]) + bgzf(p3[1]) + member(p3[2], name=b"plain") + bgzf(p3[0]) + bgzf(p3[2]) + EOF_BLOCK, R.OK,
        p3[0] + p3[1] + p3[2] + p3[0] + p3[2])

    # ---- lying BGZF: the members before the lie come back, the status is never 0
    parts = LIE_PARTS
    ms = [bgzf(p) for p in parts]

    def lie(name, k, m, expect, eof=True):
        file = b"".join(ms[:k]) + m + b"".join(ms[k + 1:]) + (EOF_BLOCK if eof else b"")
        assert len(file) < 30000  # BSIZE 0xFFFF points past the end from every member
        add("lie-%s-member-%d%s" % (name, k, "" if eof else "-last"), file, expect, b"".join(parts))

    for k in (0, 2, 3):
        p, eof = parts[k], k != 3
        lie("bsize-one-less", k, bgzf(p, delta=-1), R.E_INFLATE, eof)
        lie("bsize-one-more", k, bgzf(p, delta=1), R.E_INFLATE, eof)
        lie("bsize-past-the-end", k, bgzf(p, bsize=0xFFFF), R.E_INFLATE, eof)
        lie("bsize-below-header", k, bgzf(p, bsize=20), R.E_INFLATE, eof)
        if k != 3:
            lie("bsize-covers-next", k, bgzf(p, delta=len(ms[k + 1])), R.E_INFLATE)
        # ISIZE: behind an understated one the next member (the EOF block, too) starts inside this one's bytes
        lie("isize-minus-1", k, _patch(ms[k], -4, "<I", len(p) - 1), RACE if eof else R.E_ISIZE, eof)
        lie("isize-0", k, _patch(ms[k], -4, "<I", 0), RACE if eof else R.E_ISIZE, eof)
        lie("isize-plus-1", k, _patch(ms[k], -4, "<I", len(p) + 1), R.E_ISIZE, eof)
        lie("isize-ffffffff", k, _patch(ms[k], -4, "<I", 0xFFFFFFFF), R.E_ISIZE, eof)
        lie("crc", k, _patch(ms[k], -8, "<I", zlib.crc32(p) ^ 0x00010000), R.E_CRC, eof)

    # ---- trailing bytes
    t = blob(900, 400)
    mt = member(t)
    for z in range(1, 21):
        add("trailing-%d-zeros" % z, mt + b"\0" * z, R.OK, t)
    add("trailing-one-byte", mt + b"x", R.E_TRAILING, t)
    add("trailing-nine-bytes-of-header", mt + b"\x1f\x8b\x08" + b"\0" * 6, R.E_TRAILING, t)
    add("trailing-twelve-bytes-cut-header", mt + b"\x1f\x8b\x08\x08" + b"\0" * 6 + b"ab", R.E_TRUNCATED, t)
    add("trailing-twelve-bytes-bad-header", mt + b"\x1f\x8b\x09" + b"\0" * 9, R.E_HEADER, t)
    add("trailing-garbage-after-zeros", mt + b"\0\0\0x", R.E_TRAILING, t)
    add("trailing-magic-after-zeros", mt + b"\0\0\0" + mt, R.E_TRAILING, t)

    # ---- caps
    c3 = [blob(6000, 500), blob(7000, 501), blob(8000, 502)]
    for label, build in (("plain", lambda p: member(p)), ("bgzf", bgzf)):
        raw = b"".join(build(p) for p in c3)
        total = sum(len(p) for p in c3)
        add("cap-exact-" + label, raw, R.OK, cap=total)
        add("cap-one-short-" + label, raw, R.E_OUTPUT_FULL, cap=total - 1)
        add("cap-0-" + label, raw, R.E_OUTPUT_FULL, cap=0)
        add("cap-ends-in-member-1-" + label, raw, R.E_OUTPUT_FULL, cap=len(c3[0]) + 5)
        add("cap-ends-at-member-2-" + label, raw, R.E_OUTPUT_FULL, cap=len(c3[0]) + len(c3[1]))
    add("cap-0-empty-member", member(b""), R.OK, cap=0)
    add("null-input", None, R.E_HEADER, cap=100)
    add("null-output", mt, R.E_HEADER, cap=None)

    # ---- damage
    dd = blob(15000, 600)
    for label, m in (("dynamic", member(dd, 9)), ("fixed", member(dd, 6, zlib.Z_FIXED)), ("stored", member(dd, 0))):
        for at in (10, 11, 12, 15, 10 + (len(m) - 18) // 2, len(m) - 10, len(m) - 9):
            add("cut-%s-at-%d" % (label, at), m[:at], CUT, dd)
            add("cut-%s-at-%d-second" % (label, at), first + m[:at], CUT, d + dd)
        for keep in range(8):
            add("trailer-%s-%d-bytes" % (label, keep), m[:len(m) - 8 + keep], R.E_TRUNCATED, dd)
            add("trailer-%s-%d-bytes-second" % (label, keep), first + m[:len(m) - 8 + keep], R.E_TRUNCATED, d + dd)
    st = member(dd, 0)  # one stored block: 01, LEN, NLEN, the bytes
    add("flip-stored-payload-bit", _patch(st, 10 + 5 + 100, "<B", st[10 + 5 + 100] ^ 0x04), R.E_CRC, dd)
    add("flip-stored-nlen-bit", _patch(st, 10 + 3, "<B", st[10 + 3] ^ 0x01), R.E_INFLATE, dd)
    add("flip-stored-payload-bit-second", first + _patch(st, 10 + 5 + 100, "<B", st[10 + 5 + 100] ^ 0x04), R.E_CRC, d + dd)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    for c in out:  # one status per case outside the two families
        assert c.expect in FAMILY_SETS or c.expect in range(8), c.name
    return out


def allowed(case):
    return FAMILY_SETS.get(case.expect) or {case.expect}


def want(case):
    """the restatement's answer for a case; a NULL entry is E_HEADER with nothing decoded (include/decode_gz.h)"""
    if case.data is None or case.cap is None:
        return R.Want({R.E_HEADER}, 0, b"", 0, None)
    return R.gunzip(case.data, case.cap)
