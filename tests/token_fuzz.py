"""TEST TOOLING: raw DEFLATE streams written bit by bit from an explicit TOKEN LIST, so a test chooses
every literal, every (length, distance) and every block boundary itself.  zlib, tools/streamgen.c and
header_fuzz.tokens_for never emit a distance above 32 767 and cannot place a match; the kernels have
their edges exactly there (TOK_MATCH's 15-bit distance field, the 32 768-byte reach of hist_buf, the
too-far check that is switched off behind the first 32 KiB, CK_HIST of the chunk tasks, the far-match
resolve).  The bit writer, the canonical codes, the random code lengths and the randomised header
coding are those of header_fuzz.

A token is
    an int 0..255            a literal byte
    (length, distance)       a match, 3 <= length <= 258, 1 <= distance <= 32 768
    Block(kind)              a block boundary; kind is "stored", "fixed" or "dynamic"
    Stop(code, nbits)        (tests/table_shapes.py only) a bit pattern of a Huffman block that the
                             reference finds no code for: written like a code, it ends the decode
and a token list starts with a Block.  A stored block holds the literals up to the next boundary
(LEN = their number, 0 included).  decode_tokens() applies a token list to a bytearray in plain
Python: the witness beside the oracle and zlib.

Only legal codes are written: complete prefix codes from header_fuzz.random_lengths (or a lone 1-bit
distance symbol under HDIST >= 2, Q6), no seeded code longer than max_len = 12 bits (Q8; a Block's
explicit lengths, which tests/table_shapes.py chooses, go up to 15 and may be incomplete), no repeat code at position
0, no run behind the last length, no symbols 286 / 287.  Every case is padded with bytes(8), so the
tail rule (Q2) and the 4-byte over-read (Q3) decide nothing.  All of it is deterministic from seeds."""
import functools
import random

from header_fuzz import (CL_ORDER, DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, BitWriter, canonical, random_lengths,
                         rle)

WINDOW = 32768
PAD = bytes(8)


class Block:
    """a block boundary: the tokens behind it, up to the next boundary, make one block of this kind;
    ll / dl: explicit code lengths of a dynamic block {symbol: length} instead of seeded random ones"""

    def __init__(self, kind, ll=None, dl=None):
        assert kind in ("stored", "fixed", "dynamic")
        self.kind, self.ll, self.dl = kind, ll, dl

    def __repr__(self):
        return f"Block({self.kind})"


class Stop:
    """`nbits` bits, written first bit first like a Huffman code, where a literal/length code (or, with
    length= a match length, the distance code behind that length) is due -- and for which the block's
    tables hold no code, or none inside the reference's probe range (Q7): the decode ends in front of
    it with good = 0"""

    def __init__(self, code, nbits, length=None):
        self.code, self.nbits, self.length = code, nbits, length

    def __repr__(self):
        return f"Stop({self.code:#x}, {self.nbits})"


class Case:
    def __init__(self, name, tokens, seed, cap=None, slack=1, max_len=12):
        self.name, self.tokens = name, tokens
        self.family = name.split("/")[0]
        self.plain, self.legal = decode_tokens(tokens)
        self.tok_bits = []  # the first bit of every token that is no Block, in order
        enc = encode(tokens, seed, max_len, self.tok_bits)
        self.raw = enc.raw + PAD
        self.data_bit0, self.n_bits, self.blocks, self.codes = enc.data_bit0, enc.n_bits, enc.blocks, enc.codes
        # Q1 / Q12: recipient_size >= max(D + 1, C) unless the case is about recipient_size itself
        self.cap = cap if cap is not None else max(len(self.plain) + slack, len(self.raw))
        assert self.cap >= len(self.raw), name
        self.damaged = False

    def __repr__(self):
        return self.name


def decode_tokens(tokens):
    """-> (bytes produced, legal).  A match that reaches in front of the first byte ends the decode
    there: legal = False and the bytes are those in front of it (Q10)."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, Block):
            continue
        if isinstance(t, Stop):
            return bytes(out), False
        if isinstance(t, tuple):
            n, d = t
            if d > len(out):
                return bytes(out), False
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                for _ in range(n):
                    out.append(out[-d])
        else:
            out.append(t)
    return bytes(out), True


class _Writer(BitWriter):
    """BitWriter that moves whole bytes out of the accumulator (streams of 100 KB stay linear)"""

    def __init__(self):
        super().__init__()
        self.done = bytearray()

    def put(self, v, nbits):
        super().put(v, nbits)
        if self.n >= 64:
            k = self.n // 8
            self.done += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def put_code(self, code, nbits):  # the same bits as BitWriter.put_code, in one step
        self.put(int(format(code, "b").zfill(nbits)[::-1], 2) if nbits else 0, nbits)

    def bitpos(self):
        return 8 * len(self.done) + self.n

    def align(self):
        if self.n % 8:
            self.put(0, 8 - self.n % 8)

    def put_bytes(self, b):
        assert self.n % 8 == 0
        self.done += super().bytes()
        self.acc, self.n = 0, 0
        self.done += b

    def bytes(self):
        return bytes(self.done) + super().bytes()


def _len_sym(n):
    k = 28 if n == 258 else max(k for k in range(28) if LEN_BASE[k] <= n)
    return k, n - LEN_BASE[k]


def _dist_sym(d):
    k = max(k for k in range(30) if DIST_BASE[k] <= d)
    return k, d - DIST_BASE[k]


_LEN_SYM = [None, None, None] + [_len_sym(n) for n in range(3, 259)]
_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_LC = canonical(_FIXED_LL)


def _put_tokens(w, toks, ll, lc, dl, dc, marks=None):
    """the symbols of one Huffman block; dl = None: the fixed 5-bit distance codes"""
    for t in toks:
        if marks is not None:
            marks.append(w.bitpos())
        if isinstance(t, Stop):
            if t.length is not None:
                ls, le = _LEN_SYM[t.length]
                w.put_code(lc[257 + ls], ll[257 + ls])
                w.put(le, LEN_EXTRA[ls])
            w.put_code(t.code, t.nbits)
        elif isinstance(t, tuple):
            ls, le = _LEN_SYM[t[0]]
            ds, de = _dist_sym(t[1])
            w.put_code(lc[257 + ls], ll[257 + ls])
            w.put(le, LEN_EXTRA[ls])
            if dl is None:
                w.put_code(ds, 5)
            else:
                w.put_code(dc[ds], dl[ds])
            w.put(de, DIST_EXTRA[ds])
        else:
            w.put_code(lc[t], ll[t])
    w.put_code(lc[256], ll[256])


def _dynamic_codes(rng, blk, toks, max_len):
    """code lengths for the symbols that occur (and a few that never do): complete codes, every
    distance length below HDIST (Q6)"""
    used_lit, used_dist = {256}, set()
    for t in toks:
        if isinstance(t, Stop):
            if t.length is not None:
                used_lit.add(257 + _LEN_SYM[t.length][0])
        elif isinstance(t, tuple):
            used_lit.add(257 + _LEN_SYM[t[0]][0])
            used_dist.add(_dist_sym(t[1])[0])
        else:
            used_lit.add(t)
    ll, dl = [0] * 286, [0] * 30
    if blk.ll is not None:
        assert used_lit <= set(blk.ll) and used_dist <= set(blk.dl)
        for s, l in blk.ll.items():
            ll[s] = l
        for s, l in blk.dl.items():
            dl[s] = l
        ul, ud = sorted(blk.ll), sorted(blk.dl)
    else:
        for _ in range(rng.randint(0, 12)):
            used_lit.add(rng.randrange(0, 286))
        for _ in range(rng.randint(0, 4)):
            used_dist.add(rng.randrange(0, 30))
        if not used_dist:
            used_dist.add(rng.randrange(0, 30))
        while len(used_lit) < 2:
            used_lit.add(rng.randrange(0, 256))
        ul, ud = sorted(used_lit), sorted(used_dist)
        for s, l in zip(ul, random_lengths(rng, len(ul), max_len)):
            ll[s] = l
        for s, l in zip(ud, random_lengths(rng, len(ud), max_len)):
            dl[s] = l
    hlit = max(257, max(ul) + 1 + (rng.randint(0, 3) if max(ul) < 282 else 0))
    hdist = max(max(ud) + 1, 2 if len(ud) == 1 else 1)
    assert all(l < hdist for l in dl) and hlit <= 286
    return ll, dl, hlit, hdist


def _put_dynamic_header(rng, w, ll, dl, hlit, hdist):
    items = rle(rng, ll[:hlit] + dl[:hdist], False)
    cl_used = sorted({s for s, _, _ in items})
    if len(cl_used) == 1:
        cl_used = sorted(set(cl_used) | {(cl_used[0] + 1) % 19})
    cll = [0] * 19
    for s, l in zip(cl_used, random_lengths(rng, len(cl_used), 7)):
        cll[s] = l
    hclen = max(4, max(k for k in range(19) if cll[CL_ORDER[k]]) + 1)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cll[CL_ORDER[k]], 3)
    clc = canonical(cll)
    for s, nb, ev in items:
        w.put_code(clc[s], cll[s])
        w.put(ev, nb)


class _Encoded:
    pass


def encode(tokens, seed, max_len=12, marks=None):
    """the raw DEFLATE stream of a token list (no padding).  .blocks = [(kind, first bit of the
    block header, bytes produced in front of it)], .data_bit0 = first bit behind the first header.
    max_len: the longest seeded random code (a Block's explicit lengths go up to 15 whatever it is);
    marks: a list that receives the first bit of every token that is no Block; .codes = per block
    (ll, dl) of a dynamic block, else None."""
    rng = random.Random(seed)
    assert isinstance(tokens[0], Block)
    groups = []
    for t in tokens:
        if isinstance(t, Block):
            groups.append((t, []))
        else:
            groups[-1][1].append(t)
    w = _Writer()
    e = _Encoded()
    e.blocks, e.codes, e.data_bit0, pos = [], [], None, 0
    for gi, (blk, toks) in enumerate(groups):
        e.blocks.append((blk.kind, w.bitpos(), pos))
        w.put(1 if gi == len(groups) - 1 else 0, 1)
        w.put({"stored": 0, "fixed": 1, "dynamic": 2}[blk.kind], 2)
        if blk.kind == "stored":
            assert all(isinstance(t, int) for t in toks) and len(toks) <= 65535
            w.align()
            w.put(len(toks), 16)
            w.put(len(toks) ^ 0xFFFF, 16)
            w.align()
            if e.data_bit0 is None:
                e.data_bit0 = w.bitpos()
            if marks is not None:
                marks.extend(w.bitpos() + 8 * k for k in range(len(toks)))
            w.put_bytes(bytes(toks))
            e.codes.append(None)
        elif blk.kind == "fixed":
            if e.data_bit0 is None:
                e.data_bit0 = w.bitpos()
            _put_tokens(w, toks, _FIXED_LL, _FIXED_LC, None, None, marks)
            e.codes.append(None)
        else:
            ll, dl, hlit, hdist = _dynamic_codes(rng, blk, toks, max_len)
            _put_dynamic_header(rng, w, ll, dl, hlit, hdist)
            if e.data_bit0 is None:
                e.data_bit0 = w.bitpos()
            _put_tokens(w, toks, ll, canonical(ll), dl, canonical(dl), marks)
            e.codes.append((ll, dl))
        pos += sum(t[0] if isinstance(t, tuple) else 0 if isinstance(t, Stop) else 1 for t in toks)
    e.n_bits = w.bitpos()
    e.raw = w.bytes()
    return e


# ------------------------------------------------------------------ pieces
def prelude(rng, n):
    """tokens for exactly n bytes that are not periodic: a few hundred seeded literals, then seeded
    matches anywhere into what exists (with literals in between).  32 KiB of history costs a few
    hundred bytes of raw stream."""
    toks, pos = [], 0
    n_lit = min(n, rng.randint(200, 400))
    while pos < n:
        if pos < n_lit or n - pos < 3 or rng.random() < 0.2:
            toks.append(rng.getrandbits(8))
            pos += 1
        else:
            length = min(rng.randint(3, 258), n - pos)
            toks.append((length, rng.randint(1, min(pos, WINDOW))))
            pos += length
    return toks


def random_tokens(rng, pos, n, p_lit=0.5):
    """about n more bytes behind pos bytes: a literal, or a match whose length is uniform over
    3..258 and whose distance is uniform over the distance CODES, then inside the code, clipped to
    the bytes produced -- far distances are as common as near ones"""
    toks, end = [], pos + n
    while pos < end:
        if pos == 0 or rng.random() < p_lit:
            toks.append(rng.getrandbits(8))
            pos += 1
        else:
            c = rng.randrange(30)
            d = min(DIST_BASE[c] + rng.getrandbits(DIST_EXTRA[c]), pos)
            length = rng.randint(3, 258)
            toks.append((length, d))
            pos += length
    return toks, pos


def _kinds(kind):
    return ("dynamic", "fixed") if kind == "fixed" else ("fixed", "dynamic")


# ------------------------------------------------------------------ families
F1_LENGTHS = (3, 4, 258, 257)  # 258 = symbol 285; 257 = symbol 284 with its top extra value but one


def f1_distance_edges():
    """every distance code at its base and at its top (32 768 for code 29) with the lengths above,
    once in a fixed and once in a dynamic block, behind a prelude of exactly `top` bytes in a block of
    the other kind: the first match at `top` reads byte 0 of the stream"""
    out = []
    for kind in ("fixed", "dynamic"):
        for c in range(30):
            rng = random.Random(1000 + c)
            base, top = DIST_BASE[c], DIST_BASE[c] + (1 << DIST_EXTRA[c]) - 1
            toks = [Block(_kinds(kind)[0])] + prelude(rng, top) + [Block(kind)]
            for n in F1_LENGTHS:
                toks += [(n, top), rng.getrandbits(8), (n, base), rng.getrandbits(8)]
            out.append(Case(f"F1/{kind}/code{c}", toks, 1100 + c))
    return out


F2_P = (1, 2, 63, 64, 65, 4095, 32767, 32768)
F2_FAR_P = (32769, 65535, 65536, 65537, 98304)


def f2_distance_equals_produced():
    """at output position P a match with distance P (reads byte 0) and one with P + 1 (Q10: good = 0,
    final = P; distance 32 769 cannot be written, so P = 32 768 has the legal form only); beyond
    32 768 the distance 32 768 at positions where the tile base is at or behind 32 768"""
    out = []
    for kind in ("fixed", "dynamic"):
        for P in F2_P:
            rng = random.Random(2000 + P)
            pre = [Block(kind)] + prelude(rng, P)
            n = rng.choice((3, 100, 258))
            out.append(Case(f"F2/{kind}/P{P}/legal", pre + [(n, P), rng.getrandbits(8)], 2100 + P))
            if P < WINDOW:
                out.append(Case(f"F2/{kind}/P{P}/q10", pre + [(n, P + 1), rng.getrandbits(8)], 2200 + P,
                                cap=max(P + 600, 64)))
        for P in F2_FAR_P:
            rng = random.Random(2300 + P)
            toks = [Block(kind)] + prelude(rng, P) + [(rng.choice((3, 100, 258)), WINDOW), rng.getrandbits(8)]
            out.append(Case(f"F2/{kind}/P{P}/far", toks, 2400 + P))
    return out


F3_DIST = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)


def f3_lengths(d):
    return sorted({n for n in (max(d + 1, 3), 2 * d, 258) if d < n <= 258 and n >= 3})


def f3_overlap():
    """length > distance around the dword, 16-byte store and wavefront widths"""
    out = []
    for kind in ("fixed", "dynamic"):
        for d in F3_DIST:
            rng = random.Random(3000 + d)
            toks = [Block(_kinds(kind)[0])] + prelude(rng, d + rng.randint(0, 300)) + [Block(kind)]
            for n in f3_lengths(d):
                toks += [(n, d)] + [rng.getrandbits(8) for _ in range(rng.randint(1, 3))]
            out.append(Case(f"F3/{kind}/d{d}", toks, 3100 + d))
    return out


def f4_dependent_chains(n_matches=2000):
    """every match copies what the match before it produced: distance = previous length, distance =
    previous length + 1, and a chain of matches at distance 32 768"""
    out = []
    for kind in ("fixed", "dynamic"):
        for var in ("prev", "prev+1", "far"):
            rng = random.Random(4000 + len(var))
            if var == "far":
                toks = [Block(kind)] + prelude(rng, WINDOW)
                for _ in range(n_matches):
                    toks.append((rng.choice((3, 4, 17, 64, 65, 258)) if rng.random() < 0.2 else rng.randint(3, 70), WINDOW))
            else:
                toks = [Block(kind)] + prelude(rng, 300)
                prev = 7
                toks.append((prev, 300))
                for _ in range(n_matches):
                    n = 258 if rng.random() < 0.05 else rng.randint(3, 90)
                    toks.append((n, prev + (var == "prev+1")))
                    prev = n
            out.append(Case(f"F4/{kind}/{var}", toks, 4100 + len(var)))
    return out


F5_CHUNKS = (1024, 3072)


def f5_tokens(seed, total=100000):
    """blocks of 200..3000 bytes, stored / fixed / dynamic in turn with empty stored blocks in
    between.  Behind the first 32 KiB every dynamic block -- the only place where a chunk task can
    start -- opens with a match at distance 32 768 and one at 32 767 whose source bytes lie in a stored
    block: a stored filler block of just the right length in front of it shifts the block to where
    that holds."""
    rng = random.Random(seed)
    toks, pos, stored = [], 0, []  # stored: [first, last) output ranges of the stored blocks
    far = 0

    def in_stored(a, b):
        return any(s <= a and b <= e for s, e in stored)

    def add_stored(n):
        nonlocal pos
        toks.append(Block("stored"))
        toks.extend(rng.getrandbits(8) for _ in range(n))
        if n:
            stored.append((pos, pos + n))
        pos += n

    k = 0
    while pos < total:
        kind = ("stored", "fixed", "dynamic")[k % 3]
        k += 1
        if kind == "stored":
            add_stored(rng.randint(1000, 3000))
            continue
        n1, n2 = rng.choice((3, 40, 258)), rng.choice((3, 129, 258))
        lead = []
        if pos >= WINDOW:
            if kind == "dynamic":
                delta = next(dl for dl in range(70000) if in_stored(pos + dl - WINDOW, pos + dl - WINDOW + n1)
                             and in_stored(pos + dl + n1 - WINDOW + 1, pos + dl + n1 - WINDOW + 1 + n2))
                add_stored(delta)  # delta = 0: an empty stored block
            if in_stored(pos - WINDOW, pos - WINDOW + n1) and in_stored(pos + n1 - WINDOW + 1, pos + n1 - WINDOW + 1 + n2):
                lead = [(n1, WINDOW), (n2, WINDOW - 1)]
                far += kind == "dynamic"
        elif rng.random() < 0.5:
            add_stored(0)
        toks.append(Block(kind))
        toks += lead
        pos += sum(t[0] for t in lead)
        body, pos = random_tokens(rng, pos, rng.randint(200, 1200))
        toks += body
    return toks, far


def f5_task_starts(case, chunk):
    """the output positions at which the chunk route starts its tasks k >= 1 for `chunk` compressed
    bytes per task: the first dynamic block header at or behind byte k * chunk, if it lies in front of
    byte (k + 1) * chunk (inflate_chunk_kernel.inc: find and bounds kernels)"""
    dyn = [(bit, pos) for kind, bit, pos in case.blocks if kind == "dynamic"]
    starts = set()
    for k in range(1, len(case.raw) // chunk + 1):
        hit = [pos for bit, pos in dyn if 8 * k * chunk <= bit < 8 * (k + 1) * chunk]
        if hit:
            starts.add(hit[0])
    return sorted(starts)


def f5_across_blocks(n=3):
    out = []
    for i in range(n):
        toks, far = f5_tokens(5000 + i)
        c = Case(f"F5/{i}", toks, 5100 + i)
        c.far_dynamic_blocks = far
        out.append(c)
    return out


F6_LIT = 0x5A


def f6_maximal_expansion(n_matches=4000):
    """a dynamic block whose literal/length code is {one literal: 2 bits, 285: 1 bit, 256: 2 bits} and
    whose distance code is two 1-bit symbols: 258 bytes for 2 bits plus the distance's extra bits.
    Distance 1, 258, 32 768, and 1 and 32 768 in turn, behind a token prelude in a fixed block."""
    out = []
    for var, dists in (("d1", (1,)), ("d258", (258,)), ("d32768", (WINDOW,)), ("alt", (1, WINDOW))):
        rng = random.Random(6000 + len(var) + dists[0])
        codes = {_dist_sym(d)[0] for d in dists}
        if len(codes) == 1:
            codes.add((min(codes) + 1) % 29)  # the second 1-bit symbol never occurs
        toks = [Block("fixed")] + prelude(rng, max(dists) if max(dists) > 1 else 0)
        toks += [Block("dynamic", ll={F6_LIT: 2, 285: 1, 256: 2}, dl={s: 1 for s in codes}), F6_LIT]
        toks += [(258, dists[j % len(dists)]) for j in range(n_matches)]
        out.append(Case(f"F6/{var}", toks, 6100 + len(var)))
    return out


F7_CROSS = (1, 2, 257, 0, -1)  # the last match crosses recipient_size by ..., ends on it, one short of it


def f7_recipient_edge():
    """F1 / F3 matches as the last token of a stream, recipient_size around the match's end.  The
    prelude is long enough for Q1 (recipient_size >= input size) to hold in every variant."""
    out = []
    for kind in ("fixed", "dynamic"):
        for d in (WINDOW, WINDOW - 1, 24577, 1, 2, 3, 16, 64):
            rng = random.Random(7000 + d)
            toks = [Block(kind)] + prelude(rng, max(d, 1500) + rng.randint(0, 200)) + [(258, d)]
            for x in F7_CROSS:
                plain_len = sum(t[0] if isinstance(t, tuple) else 1 for t in toks[1:])
                out.append(Case(f"F7/{kind}/d{d}/cross{x}", toks, 7100 + d, cap=plain_len - x))
    return out


def f8_random(inflate, n=300, first=0):
    """seeded random token lists of 2..120 KB output with all three block types at random
    boundaries; every fifth gets one bit flipped behind its first block header, and the oracle
    (inflate(raw, cap, want_stats=True)) decides: a flipped stream on which the reference is in
    undefined behaviour (ub_flags != 0) is made again from the next seed until it is clean."""
    out = []
    seed = 8000 + 1000 * first
    for i in range(first, first + n):
        while True:
            seed += 1
            rng = random.Random(seed)
            total = int(2000 * 60 ** rng.random())
            toks, pos = [], 0
            while pos < total:
                kind = rng.choice(("stored", "fixed", "dynamic"))
                toks.append(Block(kind))
                n_blk = rng.choice((0, 1, 50, 700, 5000, 30000)) if rng.random() < 0.5 else rng.randint(1, 20000)
                n_blk = min(n_blk, total - pos + 300)
                if kind == "stored":
                    n_blk = min(n_blk, 3000)
                    toks.extend(rng.getrandbits(8) for _ in range(n_blk))
                    pos += n_blk
                else:
                    body, pos = random_tokens(rng, pos, n_blk)
                    toks += body
            c = Case(f"F8/{i}", toks, seed, slack=rng.choice((1, 2, 64, 1000)))
            if i % 5 == 4:
                b = bytearray(c.raw)
                bit = rng.randrange(c.data_bit0, c.n_bits)
                b[bit // 8] ^= 1 << (bit % 8)
                c.raw, c.damaged, c.name = bytes(b), True, f"F8/{i}/flipped"
                if inflate(c.raw, c.cap, want_stats=True)[3].ub_flags:
                    continue
            out.append(c)
            break
    return out


@functools.lru_cache(maxsize=None)
def fixed_families():
    """F1..F7 at full size, built once per process"""
    return {"F1": f1_distance_edges(), "F2": f2_distance_equals_produced(), "F3": f3_overlap(),
            "F4": f4_dependent_chains(), "F5": f5_across_blocks(), "F6": f6_maximal_expansion(),
            "F7": f7_recipient_edge()}


def golden_subset():
    """about 40 cases for the reference-made fixture (tests/golden/corpus_tokens.json): distance
    edges, distance = bytes produced on both sides, overlap, one stream across blocks, and the
    recipient edge where the reference has an answer -- it has no output bound of its own (Q12), so
    the variants that cross recipient_size are left to the oracle"""
    f = fixed_families()
    pick = [c for c in f["F1"] if c.name.split("/")[2] in ("code0", "code3", "code16", "code28", "code29")]
    pick += [c for c in f["F2"] if c.name.split("/")[2] in ("P1", "P64", "P32767", "P32768", "P65536")]
    pick += [c for c in f["F3"] if c.name.split("/")[2] in ("d1", "d3", "d17", "d64")][:6]
    pick += f["F5"][:1]
    pick += [c for c in f["F7"] if c.name.split("/")[2] in ("d32768", "d1") and c.name.endswith(("cross0", "cross-1"))]
    return pick
