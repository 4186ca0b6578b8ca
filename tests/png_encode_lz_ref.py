"""TEST TOOLING: a numpy restatement of level 3 of the PNG encode (include/debig_hip.h: the rule under
debig_hip_png_encode_lz_batch; csrc/png_encode_lz_kernel.inc): the match length L(p) of every position of a chunk, the walk with its
one-step deferral, and fixed_block() -- the exact bytes of a task that writes its tokens in the fixed code.  The codes, the three
sizes, the choice, the dynamic block and the bit reader are level 2's (png_encode_dyn_ref).  A token is an int (a literal byte) or
(length, distance).  Nothing here looks at the kernels' code.

THE RULE.  Chunks, the window and the table are level 1's: a table of 4096 entries indexed by ((b0 | b1 << 8 | b2 << 16) * 0x9E3779B1
mod 2^32) >> 20 holds position + 1 of the LATEST position inserted; before a chunk's first step it holds the up to 32768 positions in
front of the chunk that have three stream bytes; the chunk is walked in steps of 64 positions, and in a step every position that
has at least three bytes left in the chunk first reads the entry of its hash and only then inserts itself.

A task carries row_stride S (0: none; else bpp < S and S + bpp <= 32768).  For position p of the chunk, gp = c0 + p and maxl =
min(258, len - p).  If maxl < 3, L(p) = 0.  Otherwise the candidates are tried in this order: distance 1; bpp, if bpp > 1; S;
S - bpp; S + bpp; the table's candidate, if it is in front of gp and within 32768.  A candidate needs gp >= d, and a distance
equal to an earlier one is skipped.  The longest match wins, ties go to the earlier candidate.  A best below 3, or of 3 farther
than 4096, is 0.

The walk is greedy with one deferral.  At an uncovered position q the token is a LITERAL when 3 <= L(q) < 16, q % 64 != 63,
q + 1 < len and L(q + 1) > L(q); otherwise it is the match of L(q) bytes, or a literal when L(q) is 0.  The check applies again at
q + 1."""
import numpy as np

from png_encode_ref import NO_STORED, slot_bytes  # noqa: F401
import png_encode_dyn_ref as D

WINDOW, MAX_MATCH, TOO_FAR, MAX_LAZY, HASH_BITS = 32768, 258, 4096, 16, 12
LEVEL = 3


def stride_ok(bpp, stride):
    """what a task's row_stride may be"""
    return stride == 0 or (bpp < stride and stride + bpp <= WINDOW)


def host_stride(width, channels, depth):
    """the row_stride the host passes for an image"""
    bpp = channels * depth // 8
    s = 1 + width * bpp
    return s if stride_ok(bpp, s) else 0


def _hashes(a):
    """the hash of every position of a that has three bytes"""
    v = a[:-2].astype(np.uint64) | (a[1:-1].astype(np.uint64) << 8) | (a[2:].astype(np.uint64) << 16)
    return (((v * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - HASH_BITS)).astype(np.int64)


def _run_lengths(eq):
    """eq (n,) bool -> (n,) the number of consecutive True from each position on"""
    n = len(eq)
    idx = np.arange(n)
    nxt = np.where(~eq, idx, n)  # the next False at or behind each position
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]
    return nxt - idx


def fixed_distances(bpp, stride):
    """the fixed candidates in the rule's order, a distance equal to an earlier one left out"""
    out = [1]
    for d in ([bpp] if bpp > 1 else []) + ([stride, stride - bpp, stride + bpp] if stride else []):
        if d not in out:
            out.append(d)
    return out


def lengths(stream, c0, ln, bpp, stride):
    """-> (L, dist): the rule's match of every position of the chunk, (ln,) int64 each; L 0: none"""
    assert stride_ok(bpp, stride) and 0 < ln <= 32768 and c0 + ln <= len(stream)
    s = np.frombuffer(bytes(stream), np.uint8)
    p = np.arange(ln)
    gp = c0 + p
    maxl = np.minimum(MAX_MATCH, ln - p)
    best, dist = np.zeros(ln, np.int64), np.zeros(ln, np.int64)
    chunk_end = c0 + ln
    for d in fixed_distances(bpp, stride):
        lo = max(c0, d)  # gp >= d
        if lo >= chunk_end:
            continue
        run = _run_lengths(s[lo:chunk_end] == s[lo - d:chunk_end - d])
        l = np.zeros(ln, np.int64)
        l[lo - c0:] = run
        l = np.minimum(l, maxl)
        win = l > best
        best[win], dist[win] = l[win], d
    # the table: what every position reads before its step inserts
    w0 = max(0, c0 - WINDOW)
    h = _hashes(s[w0:]) if len(s) - w0 >= 3 else np.zeros(0, np.int64)  # h[q - w0]: position q, where q + 2 < the stream's length
    table = np.zeros(1 << HASH_BITS, np.int64)
    front = np.arange(w0, min(c0, w0 + len(h)))
    np.maximum.at(table, h[front - w0], front + 1)
    cand = np.zeros(ln, np.int64)
    for base in range(0, ln, 64):
        q = np.arange(base, min(base + 64, ln))
        q = q[maxl[q] >= 3]
        if len(q):
            cand[q] = table[h[c0 + q - w0]]
            np.maximum.at(table, h[c0 + q - w0], c0 + q + 1)
    for i in np.nonzero((cand > 0) & (maxl >= 3))[0]:
        at = int(cand[i]) - 1
        d = int(gp[i]) - at
        if d < 1 or d > WINDOW or best[i] >= maxl[i]:
            continue
        m = int(maxl[i])
        ne = np.nonzero(s[at:at + m] != s[gp[i]:gp[i] + m])[0]
        l = int(ne[0]) if len(ne) else m
        if l > best[i]:
            best[i], dist[i] = l, d
    drop = (maxl < 3) | (best < 3) | ((best == 3) & (dist > TOO_FAR))
    best[drop], dist[drop] = 0, 0
    return best, dist


def walk(stream, c0, ln, L, dist):
    """-> (tokens, the positions where a match was deferred)"""
    out, deferred, q = [], [], 0
    while q < ln:
        l = int(L[q])
        if 3 <= l < MAX_LAZY and q % 64 != 63 and q + 1 < ln and L[q + 1] > l:
            deferred.append(q)
            l = 0
        if l:
            out.append((l, int(dist[q])))
            q += l
        else:
            out.append(stream[c0 + q])
            q += 1
    return out, deferred


def tokens(stream, c0, ln, bpp, stride):
    L, dist = lengths(stream, c0, ln, bpp, stride)
    return walk(stream, c0, ln, L, dist)[0]


def token_words(tokens):
    """the token row's words: a literal's byte, or bit 31 | (length - 3) << 16 | distance - 1"""
    return [0x80000000 | ((t[0] - 3) << 16) | (t[1] - 1) if isinstance(t, tuple) else t for t in tokens]


def fixed_block(tokens, last):
    """the exact bytes of a task that writes `tokens` in the fixed code (RFC 1951 3.2.6: literals 0 .. 143 are 8 bits from 00110000,
    144 .. 255 9 bits from 110010000, 256 .. 279 7 bits from 0000000, 280 .. 287 8 bits from 11000000; distances 5 bits)"""
    def ll(w, s):
        if s < 144:
            w.code(0x30 + s, 8)
        elif s < 256:
            w.code(0x190 + s - 144, 9)
        elif s < 280:
            w.code(s - 256, 7)
        else:
            w.code(0xC0 + s - 280, 8)

    w = D._Writer()
    w.put(int(bool(last)), 1)
    w.put(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            s, eb, ex = D.len_symbol(t[0])
            ll(w, s)
            w.put(ex, eb)
            d, eb, ex = D.dist_symbol(t[1])
            w.code(d, 5)
            w.put(ex, eb)
        else:
            ll(w, t)
    ll(w, 256)
    assert w.n == D.sizes(tokens, 0, last)[1]
    if not last:
        w.put(0, 3)
        w.put(0, -w.n % 8)
        w.put(0xFFFF0000, 32)
    return w.bytes()


def stored_block(chunk, last):
    n = len(chunk)
    return bytes([int(bool(last))]) + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + bytes(chunk) + (b"" if last else b"\x00\x00\x00\xff\xff")


def task_bytes(stream, c0, ln, bpp, stride, last, flags=0, slot_cap=None):
    """-> (the task's bytes, "dynamic" / "fixed" / "stored", its tokens)"""
    toks = tokens(stream, c0, ln, bpp, stride)
    what = D.choice(toks, ln, last, flags, slot_cap)
    data = D.dynamic_block(toks, last) if what == "dynamic" else fixed_block(toks, last) if what == "fixed" else stored_block(stream[c0:c0 + ln], last)
    return data, what, toks
