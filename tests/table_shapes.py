"""TEST TOOLING: DEFLATE streams whose HUFFMAN TABLES have a chosen shape, on top of tests/token_fuzz.py.

Every inflate kernel decodes a symbol by one of four routes through the tables of the current block
(debigulator_amd/csrc/inflate_kernel.inc: CodeTabsT, build_code, huff_slow): a hit in the direct table
(DIRECT), a link into a second-level table of 2^k entries (LINK(k)), the canonical probe when the
second-level tables do not fit (SLOW), or no code at all, which fails the stream.  zlib and the seeded
random codes of token_fuzz reach these routes by chance; the families here reach them on purpose, and
classify() -- a plain-Python model of the documented allocation rule -- proves it (the CENSUS of
tests/test_table_shapes_cpu.py).  The model is used for nothing else: every expected byte comes from
token_fuzz.decode_tokens, the oracle, zlib and the reference-made tests/golden/corpus_tables.json.

A geometry is (bits of the literal/length direct table, bits of the distance direct table, entries of
the second-level area, most index bits a link may have).  GEOMETRIES lists the two the kernels are built
with, STRUCT_GEOMETRY which LDS struct has which, WIDTH_GEOMETRY which waves_per_stream code
(tests/test_gpu_inflate.py: WIDTHS) decodes with which; test_geometry_list_matches_the_sources reads the
same facts out of the .inc files.

Why the 11-bit / 1024-entry geometry has no SLOW route (unreachable(), asserted by the census).  The
codes of one length L are consecutive integers, so n_L of them touch at most ceil(n_L / 2^(L-pb)) + 1
table-index prefixes, and a run that ends at length L takes 2^(L-pb) entries: a code's runs take at most
n_long + 2 * sum(2^(L-pb) for the long lengths L present) entries.  With 286 + 30 symbols that is at most
286 + 2 * (2+4+8+16) = 346 behind an 11-bit table and 30 + 2 * (2+...+64) = 282 behind the 9-bit one, 628
of 1024; and no code is more than 6 bits longer than the 9-bit table.  Behind the 10-bit table the same
bound is 286 + 2 * 62 = 410 of 256: reachable, and T3 reaches it.

All of it is seeded and deterministic; every stream is padded with token_fuzz.PAD.  Every case of T1..T4
and T6 starts with a literal 0, so its plaintext is also ONE image row of filter type 0 (png_arm).  The
48-bit token needs a distance above 16 384, so the cases that hold it start with 24 700 zero bytes from a
fixed block of a hundred matches; every other case of T1..T5 stays within a few KB of output."""
import collections
import functools
import random

import token_fuzz as tf
from token_fuzz import Block, Case, Stop

Geometry = collections.namedtuple("Geometry", "lit dist cap max_k")
GEOMETRIES = {"g10": Geometry(10, 9, 256, 6), "g11": Geometry(11, 9, 1024, 6)}
# the LDS structs that hold a CodeTabsT, and the two kernels that borrow one
STRUCT_GEOMETRY = {"WaveLdsT<1>": "g10", "WaveLdsT<2>": "g11", "WaveLdsT<4>": "g11", "WaveLdsT<8>": "g11",
                   "ScanLds": "g10", "StrandLds": "g10", "chunk kernel": "g10", "fused PNG kernel": "g10"}
# waves_per_stream code -> geometries its streams may be decoded with (0x41 / 0x42: large streams 4-wide beside small
# ones 1- / 2-wide; 0x10, 0x11, 0x20: ScanLds; 0x12, 0x13: StrandLds)
WIDTH_GEOMETRY = {1: ("g10",), 2: ("g11",), 4: ("g11",), 8: ("g11",), 0x41: ("g10", "g11"), 0x42: ("g11",),
                  0x10: ("g10",), 0x11: ("g10",), 0x12: ("g10",), 0x13: ("g10",), 0x20: ("g10",)}
SEG_BYTES = 68        # inflate_kernel.inc: the scan's segment
WIN_BYTES = 64 * 68   # SegCfg<1>::WIN, the staged window of the one-wavefront, split and chunk scans
ST_SEG_MIN, ST_SEG_MAX = 64, 768  # inflate_strand_kernel.inc: the strand scan's segment length lies between them

DIRECT, SLOW, OUT_OF_RANGE = "DIRECT", "SLOW", "OUT_OF_RANGE"
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def LINK(k):
    return f"LINK({k})"


# ------------------------------------------------------------------ the model
def probe_range(lens):
    """Q7: (qmin, qmax) of the reference's if / else-if update in symbol order"""
    qmin, qmax = 9999, 1
    for l in lens:
        if l:
            if l < qmin:
                qmin = l
            elif l > qmax:
                qmax = l
    return qmin, qmax


def _classify_one(lens, pb, cap, max_k, running):
    """one code: {symbol: route}, the second-level entries taken afterwards, and the runs
    [(route, [symbols in canonical order])]"""
    qmin, qmax = probe_range(lens)
    codes = tf.canonical(lens)
    route, runs, cur = {}, [], None
    for l, s in sorted((l, s) for s, l in enumerate(lens) if l):
        if l < qmin or l > qmax:
            route[s] = OUT_OF_RANGE
        elif l <= pb:
            route[s] = DIRECT
        else:
            pre = codes[s] >> (l - pb)
            if cur is None or cur[0] != pre:
                cur = [pre, l, []]
                runs.append(cur)
            cur[1] = l  # lengths do not decrease in canonical order: the last code knows the table size
            cur[2].append(s)
    out = []
    for pre, last, syms in runs:
        k = last - pb
        base, running = running, running + (1 << k)
        r = LINK(k) if base + (1 << k) <= cap and k <= max_k else SLOW
        for s in syms:
            route[s] = r
        out.append((r, syms))
    return route, running, out


def classify(ll, dl, geometry, want_runs=False):
    """-> ({literal/length symbol: route}, {distance symbol: route}); a route is DIRECT, LINK(k), SLOW or
    OUT_OF_RANGE.  The allocation rule of build_code: canonical order, the runs of codes that share
    their first table-index bits, a run's table size from its last code, runs allocated in order with
    the distance code behind the literal/length code, a run that does not fit (or needs more than max_k
    bits) and every later one to SLOW, codes outside Q7's probe range out of the tables altogether."""
    g = geometry
    lit, used, lruns = _classify_one(list(ll), g.lit, g.cap, g.max_k, 0)
    used = min(used, g.cap) if max(ll) > g.lit else 0  # CodeTabsT::sub_used
    dist, _, druns = _classify_one(list(dl), g.dist, g.cap, g.max_k, used) if dl is not None else ({}, 0, [])
    return (lit, dist, lruns, druns) if want_runs else (lit, dist)


def has_code(lens, pattern, nbits=15):
    """does a code inside Q7's probe range start the `nbits` bits of `pattern` (first bit = top bit)?"""
    qmin, qmax = probe_range(lens)
    codes = tf.canonical(lens)
    return any(l and qmin <= l <= qmax and l <= nbits and pattern >> (nbits - l) == codes[s] for s, l in enumerate(lens))


def entries_bound(n_syms, pb):
    """an upper bound of the second-level entries one code can take (module docstring)"""
    return n_syms + 2 * sum(1 << (L - pb) for L in range(pb + 1, 16))


def unreachable(geometry):
    """True when no set of lengths over 286 + 30 symbols sends a symbol to SLOW in this geometry"""
    g = geometry
    return entries_bound(286, g.lit) + entries_bound(30, g.dist) <= g.cap and 15 - min(g.lit, g.dist) <= g.max_k


def decoded_symbols(case):
    """[(block index, class, symbol, first bit of the token, (ll, dl))] for every symbol a decoder takes
    out of the Huffman blocks of `case`, end-of-block included, up to a Stop; class is lit, len, eob or
    dist.  Fixed blocks give their literal/length symbols only (their distances are five plain bits)."""
    out, bi, k = [], -1, 0
    codes, stopped = None, False
    toks = case.tokens
    for i, t in enumerate(toks):
        if isinstance(t, Block):
            bi += 1
            kind = t.kind
            codes = case.codes[bi] if kind == "dynamic" else (FIXED_LL, None) if kind == "fixed" else None
            continue
        bit = case.tok_bits[k]
        k += 1
        if stopped or codes is None:
            continue
        if isinstance(t, Stop):
            if t.length is not None:
                out.append((bi, "len", 257 + tf._LEN_SYM[t.length][0], bit, codes))
            out.append((bi, "stop", t, bit, codes))
            stopped = True
            continue
        if isinstance(t, tuple):
            out.append((bi, "len", 257 + tf._LEN_SYM[t[0]][0], bit, codes))
            if codes[1] is not None:
                out.append((bi, "dist", tf._dist_sym(t[1])[0], bit, codes))
        else:
            out.append((bi, "lit", t, bit, codes))
        if i + 1 == len(toks) or isinstance(toks[i + 1], Block):
            out.append((bi, "eob", 256, None, codes))
    return out


# ------------------------------------------------------------------ pieces
LEN0 = (257, 258, 259, 260, 261, 262, 263, 264, 285)  # length symbols without extra bits
LEN5 = (281, 282, 283, 284)                            # ... with five


def complete(req, pool):
    """req = {symbol: length} with Kraft sum <= 1, made complete with symbols of `pool` (taken in order)"""
    units = 32768 - sum(1 << (15 - l) for l in req.values())
    assert units >= 0
    out, pool = dict(req), [s for s in pool if s not in req]
    for l in range(1, 16):
        if units & (1 << (15 - l)):
            out[pool.pop(0)] = l
    assert sum(1 << (15 - l) for l in out.values()) == 32768
    return out


def ladder_dist(depth=15, rot=0, top=(28, 29)):
    """distance lengths 1, 2, ..., depth, depth: symbols 0..depth-2 in rotated order, `top` for the two
    longest -- every code longer than the table shares ONE prefix (a run with k = depth - 9)"""
    n = depth - 1
    dl = {s: 1 + (s + rot) % n for s in range(n)}
    dl[top[0]], dl[top[1]] = depth, depth
    return dl


SHORT_DIST = {0: 2, 1: 2, 2: 2, 3: 2}
ZEROS = [Block("fixed"), 0, (258, 1), (41, 1)]  # 300 bytes of history in front of the block under test


def zeros(n):
    """a fixed block that produces n >= 4 zero bytes: one literal, one overlapping match, then matches at distance 258"""
    toks, n = [Block("fixed"), 0], n - 1
    while n:
        m = min(258, n) if n - min(258, n) == 0 or n - min(258, n) >= 3 else n - 3
        toks.append((m, 1 if len(toks) == 2 else 258))
        n -= m
    return toks


def every_symbol(rng, ll, dl, pos, lead=(0,), skip=(), dist_cap=None):
    """tokens that decode EVERY symbol of the two codes at least once, in seeded order: each literal, each
    length symbol as a match (its extra bits seeded), the distance symbols in turn at a seeded distance
    inside the code, clipped to the bytes produced.  -> (tokens, bytes produced)"""
    toks = list(lead)
    pos += len(toks)
    lits = [s for s in ll if s < 256 and s not in skip]
    lens = [s for s in ll if s > 256 and s not in skip]
    rng.shuffle(lits)
    rng.shuffle(lens)
    dsyms = sorted(s for s in dl if s not in skip) if dl else []
    todo = list(dsyms)
    while lits or lens:
        if lens and (not lits or rng.random() < 0.4):
            s = lens.pop() - 257
            n = min(tf.LEN_BASE[s] + rng.getrandbits(tf.LEN_EXTRA[s]), 257 if s == 27 else 258)
            ok = [d for d in (todo or dsyms) if tf.DIST_BASE[d] <= min(pos, dist_cap or pos)]
            d = ok[0] if todo else rng.choice(ok)
            if d in todo:
                todo.remove(d)
            dd = min(tf.DIST_BASE[d] + rng.getrandbits(tf.DIST_EXTRA[d]), pos)
            toks.append((n, dd))
            pos += n
        else:
            toks.append(lits.pop())
            pos += 1
    while todo:  # distance symbols left over: more matches through the first length symbol
        d = todo.pop(0)
        assert tf.DIST_BASE[d] <= pos, d
        s = min(x for x in ll if x > 256) - 257
        toks.append((tf.LEN_BASE[s], tf.DIST_BASE[d]))
        pos += tf.LEN_BASE[s]
    return toks, pos


# ------------------------------------------------------------------ T1 ladder
def ladder_lit(j, second15=200):
    """lengths 1..15 and a second 15: literal 0 has 1 bit, literals 1..9 have 2..10; the codes of 11..15
    bits are, rotating with j, a literal, a length symbol without extra bits, one with five, end-of-block
    and another literal -- all in ONE run behind either table"""
    ll = {s: s + 1 for s in range(10)}
    for i, L in enumerate(range(11, 16)):
        ll[(100 + L, LEN0[i], LEN5[i % 4], 256, 120 + L)[(i + j) % 5]] = L
    ll[second15] = 15
    return ll


def t1_ladder():
    out = []
    for j in range(5):
        rng = random.Random(11000 + j)
        ll, dl = ladder_lit(j), ladder_dist(15, j)
        body, _ = every_symbol(rng, ll, dl, 24700, skip=(28, 29))
        n = tf.LEN_BASE[min(s for s in ll if s > 256) - 257]
        toks = zeros(24700) + [Block("dynamic", ll=ll, dl=dl)] + body + [(n, 16385 + j), (n, 24577 + 3 * j)]
        out.append(Case(f"T1/ladder/{j}", toks, 11100 + j))
    # the longest token DEFLATE allows: a 15-bit length code, 5 extra bits, a 15-bit distance code, 13 extra bits, with
    # its first bit at every phase of a byte (j = 3 puts a five-extra-bit length symbol at 15 bits)
    ll, dl = ladder_lit(3), ladder_dist(15, 3)
    sym5 = next(s for s in LEN5 if ll.get(s) == 15)
    n5 = tf.LEN_BASE[sym5 - 257]
    for ph in range(8):
        toks = zeros(24700) + [Block("dynamic", ll=ll, dl=dl)] + [0] * (ph + 1)
        toks += [(n5 + 31, 16385 + 8191), 7, (n5, 24577), 0, (n5 + 21, 16385 + 0x1555)]
        out.append(Case(f"T1/tok48/{ph}", toks, 11200))
    # Q8: more than 500 long-code probe slots in one block -- the reference's asserting build dies, build B answers
    ll, dl = ladder_lit(0), ladder_dist(15, 0)
    lit15 = [s for s, l in ll.items() if l == 15 and s < 256]
    toks = ZEROS + [Block("dynamic", ll=ll, dl=dl), 0] + [lit15[k % len(lit15)] for k in range(260)]
    out.append(Case("T1/q8", toks, 11300))
    return out


# ------------------------------------------------------------------ T2 every k
def runs_lit(pb, odd, eob_len, rot=0):
    """a literal/length code whose long runs end at EVERY length pb+1..15: 2^(L-pb) codes of each long
    length L -- one full run per length -- or, odd, one more, so that a run starts with the shorter code
    and the table size comes from its longer ones.  Each long class holds literals (its first members) and
    two length symbols (its last); end-of-block has eob_len bits."""
    req, lit, lens = {0: 1}, 16 + rot, [257 + (k * 7 + rot) % 29 for k in range(29)]
    assert len(set(lens)) == 29
    if eob_len <= pb:
        req[256] = eob_len
    for L in range(pb + 1, 16):
        n = (1 << (L - pb)) + (1 if odd else 0)
        syms = [lens.pop(), lens.pop()] + ([256] if L == eob_len else [])
        while len(syms) < n:
            syms.append(lit)
            lit += 1
        for s in syms:
            req[s] = L
    assert lit <= 256
    return complete(req, list(range(1, 16)) + list(range(lit, 256)))


def t2_every_k():
    """per geometry and variant one stream of six blocks (and each block of the `full` variant alone): block b has end-of-block in the literal run with
    k = b (in the direct table once b exceeds the geometry's longest link) and a distance ladder of depth
    9 + b, whose long codes are one run with k = b"""
    out = []
    for gname, g in GEOMETRIES.items():
        for odd in (0, 1):
            rng = random.Random(12000 + g.lit + odd)
            toks, pos = list(ZEROS), 300
            for b in range(1, 7):
                ll = runs_lit(g.lit, odd, g.lit + b if g.lit + b <= 15 else 4 + b, rot=b)
                dl = ladder_dist(9 + b, b, top=(14, 15))
                body, pos = every_symbol(rng, ll, dl, pos)
                toks += [Block("dynamic", ll=ll, dl=dl)] + body
                if not odd:  # the block alone as well
                    alone, _ = every_symbol(rng, ll, dl, 300)
                    out.append(Case(f"T2/{gname}/full/b{b}", list(ZEROS) + [Block("dynamic", ll=ll, dl=dl)] + alone,
                                    12200 + 10 * g.lit + b))
            out.append(Case(f"T2/{gname}/{'odd' if odd else 'full'}", toks, 12100 + g.lit + odd))
    return out


# ------------------------------------------------------------------ T3 capacity (the 10-bit / 256-entry geometry)
def cap_lit(arm):
    """literal/length lengths of a T3 arm; {1, 2, 3} bits for literals 0, 1, 2 and, by arm,
    exact    256 x 11 bits: 128 runs of 2 entries fill sub_tab to exactly 256
    over1    254 x 11 + 4 x 12: the run of four 12-bit codes would end at 258 -- 4 symbols SLOW
    over2    251 x 11 + 6 x 12 + 8 x 13: 125 runs, then {11, 12, 12} ends at exactly 254 and fits, {12 x 4} would end
             at 258 and {13 x 8} lies behind it: 12 symbols SLOW, the smallest run that can overflow and a later one
    fit192   192 x 11 and a 5-bit code: 192 entries, exactly the 64 a distance ladder needs are left
    miss194  194 x 11 and 31 x 10: 194 entries, the distance ladder's 64 do not fit
    `eob_long`: end-of-block among the longest codes (else among the 11-bit ones)"""
    counts = {"exact": {11: 256}, "over1": {11: 254, 12: 4}, "over2": {11: 251, 12: 6, 13: 8}, "fit192": {11: 192, 5: 1},
              "miss194": {11: 194, 10: 31}}[arm.split("+")[0]]
    req = {0: 1, 1: 2, 2: 3}
    lits, lens = list(range(3, 256)), list(range(257, 286))
    eob_at = max(counts) if arm.endswith("+eob") else 11
    for L in sorted(counts, reverse=True):  # the long classes first: literals, length symbols, end-of-block in one
        syms = [256] if L == eob_at else []
        if L > 11:
            syms += [lens.pop(0) for _ in range(max(1, counts[L] // 3))]
        while len(syms) < counts[L]:
            syms.append(lits.pop(0) if lits and (L != 11 or len(lens) < counts[L] - len(syms)) else lens.pop(0))
        for s in syms:
            req[s] = L
    assert sum(1 << (15 - l) for l in req.values()) == 32768, arm
    return req


T3_ARMS = (("exact", "short"), ("over1", "short"), ("over1+eob", "short"), ("over2", "short"), ("over2+eob", "ladder"),
           ("exact", "ladder"), ("fit192", "ladder"), ("miss194", "ladder"))


def t3_block(rng, lit_arm, dist_arm, pos, rot=0):
    ll = cap_lit(lit_arm)
    dl = dict(SHORT_DIST) if dist_arm == "short" else ladder_dist(15, rot, top=(14, 15))
    body, pos = every_symbol(rng, ll, dl, pos)
    return [Block("dynamic", ll=ll, dl=dl)] + body, pos


def t3_capacity():
    out = []
    for k, (la, da) in enumerate(T3_ARMS):
        rng = random.Random(13000 + k)
        blk, _ = t3_block(rng, la, da, 300, rot=k)
        out.append(Case(f"T3/{la}/{da}", list(ZEROS) + blk, 13100 + k))
    return out


def long_arm(name, tail, seed, n_hist=50000, n_blocks=8, n_syms=400):
    """40..70 KB of seeded history, then n_blocks blocks of the overflowing code with n_syms long-code symbols each
    (11..13 bits: none of them costs a probe slot of Q8), then `tail`: several windows and tiles, and at 1024 compressed
    bytes per task several chunk tasks"""
    rng = random.Random(seed)
    toks = [Block("fixed"), 0] + tf.prelude(rng, n_hist - 1)
    ll = cap_lit("over2+eob")
    dl = ladder_dist(15, 5, top=(14, 15))
    longs = [s for s, l in ll.items() if l >= 11 and s != 256]
    for _ in range(n_blocks):
        toks.append(Block("dynamic", ll=ll, dl=dl))
        for _ in range(n_syms):
            s = rng.choice(longs)
            if s < 256:
                toks.append(s)
            else:
                d = rng.choice(sorted(dl))
                toks.append((min(tf.LEN_BASE[s - 257] + rng.getrandbits(tf.LEN_EXTRA[s - 257]), 257 if s == 284 else 258),
                             tf.DIST_BASE[d] + rng.getrandbits(tf.DIST_EXTRA[d])))
    return Case(name, toks + tail, seed + 1)


# ------------------------------------------------------------------ T4 block sequences
T4_KINDS = ("deep", "overflowing", "shallow", "fixed", "stored", "onedist")


def t4_block(kind, second, rng, pos):
    """one block of `kind`; second = 1: the form a kind takes as the SECOND block of a pair -- other lengths over other
    symbols, so that the bit patterns it decodes index direct-table slots, link slots, SLOW marks and second-level
    ranges that the first form used differently (the census counts the changed slots)"""
    if kind == "deep":
        ll, dl = runs_lit(10 + second, second, 15 - second, rot=3 + 5 * second), ladder_dist(15 - second, second, top=(14, 15))
    elif kind == "overflowing":
        ll, dl = cap_lit(("over2+eob", "over1")[second]), ladder_dist(15 - 2 * second, 3 + second, top=(14, 15))
    elif kind == "shallow":  # longest code 3 bits or less: mask[] shrinks below the tables
        ll = ({0: 1, 77: 2, 256: 3, 264: 3}, {0: 2, 33: 2, 256: 2, 150: 3, 258: 3})[second]
        dl = ({0: 1, 3: 1}, {0: 1, 1: 2, 2: 3, 5: 3})[second]
    elif kind == "onedist":  # the lone 1-bit distance symbol under HDIST >= 2 (Q6), as token_fuzz writes it
        ll = complete({0: 2, 256: 5 + second, 257 + second: 4, 270: 9}, [90 + 3 * k + second for k in range(40)])
        dl = {second: 1}
    elif kind == "fixed":
        body, pos = every_symbol(rng, {s: 1 for s in list(range(second, 256, 2)) + list(range(257, 286))},
                                 {d: 5 for d in range(17)}, pos)
        return [Block("fixed")] + body, pos
    else:  # stored; the second form is LEN = 0 and then a few bytes in a block of their own
        n = 0 if second else 37
        toks = [Block("stored")] + [0] + [rng.getrandbits(8) for _ in range(n)]
        if second:
            toks = [Block("stored")] + toks
        return toks, pos + n + 1
    body, pos = every_symbol(rng, ll, dl, pos)
    return [Block("dynamic", ll=ll, dl=dl)] + body, pos


def t4_sequences():
    out = []
    for a in T4_KINDS:
        for b in T4_KINDS:
            rng = random.Random(14000 + 7 * T4_KINDS.index(a) + T4_KINDS.index(b))
            t1, pos = t4_block(a, 0, rng, 300)
            t2, pos = t4_block(b, 1, rng, pos)
            out.append(Case(f"T4/pair/{a}-{b}", list(ZEROS) + t1 + t2, 14100 + len(out)))
    for name, order in (("all6", T4_KINDS), ("all6rev", T4_KINDS[::-1])):
        rng = random.Random(14500 + len(name))
        toks, pos = list(ZEROS), 300
        for k, kind in enumerate(order):
            t, pos = t4_block(kind, k % 2, rng, pos)
            toks += t
        out.append(Case(f"T4/{name}", toks, 14600 + len(name)))
    return out


# ------------------------------------------------------------------ T5 incomplete codes and Q7
def _drop_last(lens):
    """one code of the longest length less: its bit pattern (all ones) has no code any more"""
    lens = dict(lens)
    L = max(lens.values())
    del lens[min(s for s, l in lens.items() if l == L and s != 256)]
    return lens


def t5_incomplete():
    """Kraft sums below 1, never above.  Per arm a `clean` stream that never sends the unused bit pattern (good = 1) and a
    `hit` stream that sends it at a chosen token (good = 0, the final size at the partial count).  Arms: the unused
    pattern inside a second-level table (lit/link, dist/link), in an empty direct slot (lit/direct, dist/direct), behind
    a SLOW mark of the 10-bit geometry (lit/slow, dist/slow); Q7 arms: a first symbol longer than every later
    non-minimum (q7/long: 15 bits against qmax = 13; q7/link: 12 against 5; q7/direct: 8 against 5; q7/dist)."""
    arms = []  # (name, literal/length lengths, distance lengths, the code the failing pattern belongs to)
    lad, dlad = ladder_lit(2), ladder_dist(15, 2, top=(14, 15))
    arms.append(("lit/link", _drop_last(lad), dlad, "lit"))
    arms.append(("dist/link", lad, _drop_last(dlad), "dist"))
    arms.append(("lit/direct", {0: 2, 9: 2, 256: 3, 257: 3}, {0: 1, 1: 1}, "lit"))
    arms.append(("dist/direct", {0: 1, 256: 2, 257: 2}, {0: 2, 1: 2, 2: 2}, "dist"))
    arms.append(("lit/slow", _drop_last(cap_lit("over2")), dict(SHORT_DIST), "lit"))
    arms.append(("dist/slow", cap_lit("exact"), _drop_last(dlad), "dist"))
    arms.append(("q7/long", {0: 15, 20: 13, 30: 13, 40: 3, 256: 2, 257: 1}, {0: 1, 1: 1}, "lit"))
    arms.append(("q7/link", {0: 12, 20: 5, 30: 5, 40: 3, 256: 2, 257: 1}, {0: 1, 1: 1}, "lit"))
    arms.append(("q7/direct", {0: 8, 20: 5, 30: 5, 40: 3, 256: 2, 257: 1}, {0: 1, 1: 1}, "lit"))
    arms.append(("q7/dist", {0: 1, 256: 2, 257: 3, 258: 3}, {2: 14, 3: 12, 4: 12, 17: 2, 18: 1}, "dist"))
    out = []
    for k, (name, ll, dl, which) in enumerate(arms):
        rng = random.Random(15000 + k)
        # a distance pattern stands behind the code's first length symbol
        length = tf.LEN_BASE[min(s for s in ll if s > 256) - 257] if which == "dist" else None
        if name.startswith("q7"):  # the code of the alphabet's first symbol, which lies outside the probe range
            code = ll if which == "lit" else dl
            oor = min(code)
            lens = [code.get(s, 0) for s in range(max(code) + 1)]
            stop, skip = Stop(tf.canonical(lens)[oor], code[oor], length), (oor,)
        else:  # fifteen ones: the pattern of the code that _drop_last took, or of one that never was
            stop, skip = Stop(0x7FFF, 15, length), ()
        body, pos = every_symbol(rng, ll, dl, 600, skip=skip, lead=(0,) if ll.get(0, 9) <= 3 else (40,))
        head = zeros(600) + [Block("dynamic", ll=ll, dl=dl)]
        out.append(Case(f"T5/{name}/clean", head + body, 15100 + k))
        cut = len(body) // 2
        hit = head + body[:cut] + [stop] + body[cut:]
        out.append(Case(f"T5/{name}/hit", hit, 15100 + k, cap=pos + 600))
    return out


# ------------------------------------------------------------------ T6 positions
T6_SPAN = 2 * SEG_BYTES * 8  # bit offsets 0 .. T6_SPAN - 1
T6_EDGE = tuple(range(-20, 21, 1))  # ... and these around the end of the first staged window


def t6_tokens(off, off2=5):
    """four probe groups.  `off` literals 0 of ONE bit in front of the first move all four by one bit each (the others sit
    behind off2 and off2 + 4 of them, and the headers of one seed are the same bits in every stream): the 48-bit token;
    a 15-bit end-of-block and the dynamic header behind it; a SLOW literal and then a LINK literal (10-bit geometry); a 15-bit literal as the last symbol in
    front of end-of-block in the stream's last bytes"""
    la, da = ladder_lit(4, second15=282), ladder_dist(15, 3)  # j = 4: end-of-block has 15 bits
    sym5 = 282
    lb = cap_lit("over1")
    slow = min(s for s, l in lb.items() if l == 12 and s < 256)
    link = min(s for s, l in lb.items() if l == 11)
    lc = ladder_lit(1)
    lit15 = max(s for s, l in lc.items() if l == 15 and s < 256)
    n5 = tf.LEN_BASE[sym5 - 257]
    toks = [Block("dynamic", ll=la, dl=da)] + [0] * off + [(n5 + 31, 16385 + 8191)]
    toks += [Block("dynamic", ll=lb, dl=dict(SHORT_DIST))] + [0] * off2 + [slow, link, 0, link, slow]
    toks += [Block("dynamic", ll=lc, dl=da)] + [0] * (off2 + 4) + [lit15]
    return toks


def t6_positions():
    out = []
    for off in range(T6_SPAN):
        out.append(Case(f"T6/off{off}", zeros(24700) + t6_tokens(off), 16000))
    # the window edge: the 48-bit token from 200 bits in front of the end of the window of 64 segments that starts with
    # the dynamic block to a few bits behind it, in steps of 7 bits -- staging starts at the 16-byte boundary below, so
    # the staged window ends up to 120 bits earlier than that (the census holds the positions to this)
    for d in T6_EDGE:
        out.append(Case(f"T6/edge{d:+d}", zeros(24700) + t6_tokens(WIN_BYTES * 8 - 473 + 7 * d, 40 + d), 16100))
    return out


# ------------------------------------------------------------------ all of them
@functools.lru_cache(maxsize=None)
def families():
    """T1..T6, built once per process (a few seconds); T3 and T6 end with their long arm"""
    f = {"T1": t1_ladder(), "T2": t2_every_k(), "T3": t3_capacity(), "T4": t4_sequences(), "T5": t5_incomplete(),
         "T6": t6_positions()}
    blk, _ = t3_block(random.Random(13900), "over1+eob", "ladder", 60000, rot=2)
    f["T3"].append(long_arm("T3/long", blk, 13910))
    f["T6"].append(long_arm("T6/long", t6_tokens(777), 16910, n_hist=44000, n_blocks=6))
    return f


Q8_CASE = "T1/q8"  # the one case on which the reference's asserting build dies (ORC_UB_LONGCODE_500)
COMPLETE = ("T1", "T2", "T3", "T4", "T6")  # the families whose codes are complete: zlib decodes them too


def long_arms():
    f = families()
    return [f["T3"][-1], f["T6"][-1]]


def golden_subset():
    """about 60 cases for tests/golden/corpus_tables.json: at least 6 per family, every T3 and every T5 arm"""
    f = families()
    t4 = [c for c in f["T4"] if c.name.split("/")[-1] in ("deep-overflowing", "overflowing-shallow", "shallow-deep",
                                                           "fixed-overflowing", "stored-deep", "onedist-overflowing",
                                                           "overflowing-onedist", "all6")]
    t6 = [c for c in f["T6"] if c.name in ("T6/off0", "T6/off7", "T6/off543", "T6/off544", "T6/off1087", "T6/edge+0",
                                           "T6/edge-1")]
    return f["T1"][:5] + [f["T1"][5], f["T1"][12], f["T1"][13]] + f["T2"] + f["T3"][:-1] + t4 + f["T5"] + t6


def png_arm():
    """[(name, raw DEFLATE, pixels)]: T2, T3 and the six-block stream of T4 as ONE-row 8-bit grey images.  Every such
    case starts with a literal 0 -- the row's filter byte -- so the pixels are the plaintext without it."""
    f = families()
    cs = f["T2"] + f["T3"][:-1] + [c for c in f["T4"] if c.name == "T4/all6"]
    assert all(c.legal and c.plain[0] == 0 for c in cs)
    return [(c.name, c.raw[:-len(tf.PAD)], c.plain[1:]) for c in cs]


def png_file(raw, pixels, ct=0):
    """a PNG of ONE row: `raw` (a DEFLATE stream of a filter byte 0 and then `pixels`) as its zlib stream.  ct = 0: 8-bit
    grey; ct = 3: the same bytes as indices into a 256-entry grey palette (the reference-compatible decode and its fused
    kernel know colour types 2, 3 and 6 only)."""
    import zlib

    import numpy as np

    import png_spec_ref as R

    zdata = b"\x78\x9c" + raw + zlib.adler32(b"\0" + pixels).to_bytes(4, "big")
    samples = np.frombuffer(pixels, dtype=np.uint8).reshape(1, -1, 1)
    return R.encode(samples, ct, 8, zdata=zdata, palette=[(i, i, i) for i in range(256)] if ct == 3 else None)


def walk(raw):
    """a plain bit-by-bit inflate of a stream somebody else made (zlib): -> [(ll, dl, literal/length symbols decoded,
    distance symbols decoded)] per dynamic block, so that classify() can say which routes such a stream reaches"""
    pos = 0

    def take(n):
        nonlocal pos
        v = 0
        for k in range(n):
            v |= ((raw[(pos + k) >> 3] >> ((pos + k) & 7)) & 1) << k
        pos += n
        return v

    def decoder(lens):
        table = {(l, c): s for s, c in tf.canonical(lens).items() for l in [lens[s]]}

        def sym():
            nonlocal pos
            c = 0
            for l in range(1, 16):
                c = (c << 1) | take(1)
                if (l, c) in table:
                    return table[(l, c)]
            raise ValueError("no code")
        return sym

    out, last = [], 0
    while not last:
        last, kind = take(1), take(2)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = take(16)
            pos += 16 + 8 * n
            continue
        if kind == 1:
            ll, dl = FIXED_LL, [5] * 30
        else:
            hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
            cl = [0] * 19
            for k in range(hclen):
                cl[tf.CL_ORDER[k]] = take(3)
            sym, lens = decoder(cl), []
            while len(lens) < hlit + hdist:
                s = sym()
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + take(2))
                else:
                    lens += [0] * (3 + take(3) if s == 17 else 11 + take(7))
            ll, dl = lens[:hlit], lens[hlit:hlit + hdist]
        lsym, dsym, ul, ud = decoder(ll), decoder(dl), set(), set()
        while True:
            s = lsym()
            ul.add(s)
            if s == 256:
                break
            if s > 256:
                take(tf.LEN_EXTRA[s - 257])
                d = dsym()
                ud.add(d)
                take(tf.DIST_EXTRA[d])
        if kind == 2:
            out.append((ll, dl, ul, ud))
    return out


def direct_slots(lens, pb, cap, max_k, running=0):
    """the model's picture of ONE direct table: {index: ("D", symbol) | ("L", base, k) | ("S",)} and the second-level
    ranges [(base, size, symbols)] -- what the census uses to show that the second block of a T4 pair indexes slots the
    first block filled differently"""
    route, _, runs = _classify_one(list(lens), pb, cap, max_k, running)
    codes = tf.canonical(lens)

    def rev(v, n):
        return int(format(v, "b").zfill(n)[::-1], 2) if n else 0

    slots, ranges = {}, []
    for s, r in route.items():
        if r == DIRECT:
            for q in range(rev(codes[s], lens[s]), 1 << pb, 1 << lens[s]):
                slots[q] = ("D", s)
    base = running
    for r, syms in runs:
        k = lens[syms[-1]] - pb
        idx = rev(codes[syms[0]] >> (lens[syms[0]] - pb), pb)
        slots[idx] = ("L", base, k) if r != SLOW else ("S",)
        if r != SLOW:
            ranges.append((base, 1 << k, tuple(syms)))
        base += 1 << k
    return slots, ranges


def token_rows(case):
    """an upper bound of the token rows the scan of a throughput route needs for `case`: a window ends with its block and
    costs a counts row plus one row per symbol of its busiest lane, and a lane is 68 bytes of the stream wherever the
    window starts -- so per Huffman block 1 + the most symbols (end-of-block included) that start inside any 544 bits,
    once per window of 64 lanes"""
    rows, k, toks = 0, 0, case.tokens
    starts = None
    for i, t in enumerate(toks + [Block("stored")]):
        if isinstance(t, Block):
            if starts:
                starts.append(starts[-1] + 1)  # end-of-block, behind the last symbol
                best = lo = 0
                for hi in range(len(starts)):
                    while starts[hi] - starts[lo] >= 8 * SEG_BYTES:
                        lo += 1
                    best = max(best, hi - lo + 1)
                rows += (1 + best) * (1 + (starts[-1] - starts[0]) // (8 * WIN_BYTES))
            starts = [] if t.kind != "stored" else None
            continue
        if starts is not None:
            starts.append(case.tok_bits[k])
        k += 1
    return rows
