"""TEST TOOLING: what debig_gunzip_batch (include/decode_gz.h) answers for ONE file, restated in plain Python with zlib as the
inflater -- the reference of tests/test_gpu_gunzip.py, itself checked on the CPU by tests/test_gunzip_ref_cpu.py.

gunzip(file, cap) -> Want(statuses, out_size, out, members):
  statuses  the set of allowed DEBIG_GZ_* codes: ONE code, except in two families where the library's answer depends on timing or on
            how far a cut stream gets before the inflate notices (`family` names it: "cut-stream", "isize-race", or None);
  out_size  what out_sizes[i] must be;
  out       the bytes that must come back: all out_size of them, or (family "isize-race") the output of the members in front of the
            failing one -- a prefix of the out_size bytes;
  members   what n_members[i] must be.

The rule, per member, in this order (the first that applies ends the file with its status; out_size and members count the members
that got past step 4, so a member that fails only its CRC-32 or ISIZE is counted and its bytes are part of the output):
  0. the header (parse_header): E_HEADER or E_TRUNCATED; after the first member, whatever follows a member is looked at first as
     trailing bytes: nothing or only zeros end the file well, fewer than 10 bytes or bytes that do not start 1f 8b are E_TRAILING
     (the output is complete), anything else must be a whole header;
  1. inflate: E_OUTPUT_FULL when the output does not fit behind the members so far, E_INFLATE for a damaged stream; a stream that
     stops short of its end is E_INFLATE or E_TRUNCATED;
  2. the 8 trailer bytes lie inside the file, else E_TRUNCATED;
  3. a "BC" subfield (BGZF: BSIZE = member size - 1) names exactly the member's size, else E_INFLATE -- also when it points past the
     end of the file or in front of the member's own trailer;
  4. the ISIZE fields of the BGZF members in front of this one (inflated by the same launch) put its output where the members
     before it really end, else E_ISIZE;
  5. CRC-32, else E_CRC;  6. ISIZE, else E_ISIZE.
A BGZF member is one whose BSIZE fits the file and leaves room for header + trailer: its input ends at BSIZE, and the member behind
it starts its output at this one's ISIZE field -- all members of such a chain are inflated at once.  An UNDERSTATED ISIZE therefore
makes the next member write over the tail of this one while its CRC-32 is taken: E_CRC or E_ISIZE ("isize-race")."""
import collections
import struct
import zlib

OK, E_HEADER, E_TRUNCATED, E_INFLATE, E_OUTPUT_FULL, E_CRC, E_ISIZE, E_TRAILING = range(8)
MAGIC = b"\x1f\x8b"
Want = collections.namedtuple("Want", "statuses out_size out members family")


def parse_header(p):
    """one member header at the start of p -> (status, header length, BGZF member size or 0), as debig_gz_parse_header"""
    if len(p) < 10:
        return (E_HEADER if len(p) >= 2 and p[:2] != MAGIC else E_TRUNCATED), 0, 0
    if p[:2] != MAGIC or p[2] != 8 or p[3] & 0xE0:
        return E_HEADER, 0, 0
    flg, o, bsize = p[3], 10, 0
    if flg & 4:  # FEXTRA
        if o + 2 > len(p):
            return E_TRUNCATED, 0, 0
        xlen = struct.unpack_from("<H", p, o)[0]
        o += 2
        if o + xlen > len(p):
            return E_TRUNCATED, 0, 0
        q = o
        while q + 4 <= o + xlen:  # subfields SI1 SI2 LEN data; one that runs past XLEN ends the walk
            sl = struct.unpack_from("<H", p, q + 2)[0]
            if q + 4 + sl > o + xlen:
                break
            if p[q:q + 2] == b"BC" and sl == 2:
                bsize = struct.unpack_from("<H", p, q + 4)[0] + 1
            q += 4 + sl
        o += xlen
    for bit in (8, 16):  # FNAME, FCOMMENT: zero-terminated
        if flg & bit:
            z = p.find(b"\0", o)
            if z < 0:
                return E_TRUNCATED, 0, 0
            o = z + 1
    if flg & 2:  # FHCRC: skipped, not verified
        if o + 2 > len(p):
            return E_TRUNCATED, 0, 0
        o += 2
    return OK, o, bsize


def _le32(b, at):
    return struct.unpack_from("<I", b, at)[0]


def gunzip(data, cap):
    pos = used = members = 0
    out = b""

    def end(statuses, family=None, prefix=None):
        st = statuses if isinstance(statuses, set) else {statuses}
        return Want(st, used, out if prefix is None else prefix, members, family)

    while True:
        # ---- the members of one launch: the next one, and behind a BGZF member the one its BSIZE points to
        chain, qpos, qused = [], pos, used
        while True:
            st, hl, bs = parse_header(data[qpos:])
            if st != OK:
                if not chain:
                    return end(st)
                break  # behind queued members: the next launch meets this header again, first
            bg = bs >= hl + 8 and qpos + bs <= len(data)
            chain.append((qpos, hl, bs, bg, qused))
            if not bg:
                break
            qused += _le32(data, qpos + bs - 4)
            qpos += bs
            if len(data) - qpos < 10 or data[qpos:qpos + 2] != MAGIC:
                break
        # ---- verdicts in member order
        for k, (p, hl, bs, bg, out_rel) in enumerate(chain):
            buf = data[p + hl:p + bs if bg else len(data)]
            room = cap - out_rel if out_rel <= cap else 0
            d = zlib.decompressobj(-15)
            try:
                plain = d.decompress(buf, room + 1)
            except zlib.error:
                return end(E_INFLATE)
            if len(plain) > room:
                return end(E_OUTPUT_FULL)
            if not d.eof:
                return end({E_TRUNCATED, E_INFLATE}, "cut-stream")
            trailer = p + hl + len(buf) - len(d.unused_data)
            if trailer + 8 > len(data):
                return end(E_TRUNCATED)
            if bs and trailer + 8 != p + bs:
                return end(E_INFLATE)
            if out_rel != used:
                return end(E_ISIZE)
            before = out
            used += len(plain)
            members += 1
            out += plain
            pos = trailer + 8
            crc_ok = _le32(data, trailer) == zlib.crc32(plain) & 0xFFFFFFFF
            isize_ok = _le32(data, trailer + 4) == len(plain) & 0xFFFFFFFF
            if k + 1 < len(chain) and chain[k + 1][4] < used:  # the next member of the launch writes into this one's bytes
                assert not isize_ok
                return end({E_CRC, E_ISIZE}, "isize-race", before)
            if not crc_ok:
                return end(E_CRC)
            if not isize_ok:
                return end(E_ISIZE)
        # ---- what follows the last verified member
        rest = data[pos:]
        if not rest.strip(b"\0"):
            return end(OK)
        if len(rest) < 10 or rest[:2] != MAGIC:
            return end(E_TRAILING)
