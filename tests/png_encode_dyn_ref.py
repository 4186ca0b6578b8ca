"""TEST TOOLING: a plain-Python restatement of level 2 of the PNG encode (include/debig_hip.h: the rule under
debig_hip_png_encode_dynamic_batch; csrc/png_encode_dynamic_kernel.inc): the length-limited code rule, the canonical codes, the
header rule, dynamic_block() -- the exact bytes of a task that writes a dynamic block --, the three sizes and the choice, and a bit
reader that lists a task's blocks of every type with their tokens.  A token is an int (a literal byte) or (length, distance).
Nothing here looks at the kernels' code."""
from png_encode_ref import _Bits, _LBASE, _LEXT, _DBASE, _DEXT, NO_STORED, slot_bytes

ONLY_DYNAMIC = 2  # DEBIG_PNG_ENCODE_ONLY_DYNAMIC
ROUND_TASKS = 2048  # DEBIG_PNG_ENCODE_ROUND_TASKS
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}


def tree_depths(counts):
    """the two-queue Huffman tree of the used symbols -> (the rule's order, the depth of every leaf along it), not limited"""
    order = sorted((s for s, c in enumerate(counts) if c > 0), key=lambda s: (counts[s], s))
    nu = len(order)
    assert nu >= 2
    w = [counts[s] for s in order]
    iw, lparent, iparent = [], [0] * nu, [0] * (nu - 1)
    li = ii = 0
    for _ in range(nu - 1):
        total = 0
        for _pick in range(2):
            if li < nu and (ii >= len(iw) or w[li] <= iw[ii]):  # a tie: the leaf goes first
                total += w[li]
                lparent[li] = len(iw)
                li += 1
            else:
                total += iw[ii]
                iparent[ii] = len(iw)
                ii += 1
        iw.append(total)
    idepth = [0] * (nu - 1)
    for j in range(nu - 3, -1, -1):
        idepth[j] = idepth[iparent[j]] + 1
    return order, [idepth[lparent[r]] + 1 for r in range(nu)]


def code_lengths(counts, limit):
    """the rule: counts -> lengths, every one 0 .. limit"""
    n = len(counts)
    lens = [0] * n
    used = [s for s in range(n) if counts[s] > 0]
    if len(used) < 2:
        for s in used:
            lens[s] = 1
        k = len(used)
        for s in range(n):
            if k >= 2:
                break
            if counts[s] == 0:
                lens[s] = 1
                k += 1
        return lens
    order, depth = tree_depths(counts)
    num = [0] * (limit + 1)
    for d in depth:
        num[min(d, limit)] += 1
    total = sum(num[l] << (limit - l) for l in range(1, limit + 1))
    while total > 1 << limit:
        num[limit] -= 1
        l = max(k for k in range(1, limit) if num[k] > 0)
        num[l] -= 1
        num[l + 1] += 2
        total -= 1
    r = 0
    for l in range(limit, 0, -1):
        for _ in range(num[l]):
            lens[order[r]] = l
            r += 1
    assert r == len(order)
    return lens


def canonical(lens):
    """RFC 1951 3.2.2: lengths -> codes (most significant bit first)"""
    top = max(lens) if lens else 0
    bl = [0] * (top + 2)
    for l in lens:
        if l:
            bl[l] += 1
    nxt, code = [0] * (top + 2), 0
    for b in range(1, top + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return out


def kraft(lens, limit):
    return sum(1 << (limit - l) for l in lens if l)


def len_symbol(length):
    """-> (symbol, extra bits, their value)"""
    k = max(i for i in range(29) if _LBASE[i] <= length) if length < 258 else 28
    return 257 + k, _LEXT[k], length - _LBASE[k]


def dist_symbol(dist):
    k = max(i for i in range(30) if _DBASE[i] <= dist)
    return k, _DEXT[k], dist - _DBASE[k]


def histograms(tokens):
    """-> (286 literal/length counts with the end of block, 30 distance counts)"""
    ll, dd = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            ll[len_symbol(t[0])[0]] += 1
            dd[dist_symbol(t[1])[0]] += 1
        else:
            ll[t] += 1
    ll[256] += 1
    return ll, dd


def header_symbols(ll_lens, d_lens):
    """-> (HLIT, HDIST, [(symbol 0 .. 18, the value of its extra bits)])"""
    hlit = max(257, 1 + max(s for s in range(286) if ll_lens[s]))
    hdist = 1 + max(s for s in range(30) if d_lens[s])
    seq = list(ll_lens[:hlit]) + list(d_lens[:hdist])
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
    return hlit, hdist, out


def plan(tokens):
    """everything the dynamic block of `tokens` is made of"""
    ll, dd = histograms(tokens)
    ll_lens, d_lens = code_lengths(ll, 15), code_lengths(dd, 15)
    hlit, hdist, hdr = header_symbols(ll_lens, d_lens)
    cl = [0] * 19
    for s, _ in hdr:
        cl[s] += 1
    cl_lens = code_lengths(cl, 7)
    hclen = max(4, 1 + max(i for i in range(19) if cl_lens[CL_ORDER[i]]))
    return {"ll": ll, "dd": dd, "ll_lens": ll_lens, "d_lens": d_lens, "hlit": hlit, "hdist": hdist, "hdr": hdr, "cl": cl, "cl_lens": cl_lens,
            "hclen": hclen}


def fixed_len(s):
    return 8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8


def sizes(tokens, chunk_len, last):
    """-> (stored bytes, fixed bits, dynamic bits): the bits with the block's three header bits and the end of block, dynamic with its
    header; no trailer"""
    p = plan(tokens)
    lext = lambda s: _LEXT[s - 257] if s >= 257 else 0  # noqa: E731
    fixed = 3 + sum(c * (fixed_len(s) + lext(s)) for s, c in enumerate(p["ll"])) + sum(c * (5 + _DEXT[d]) for d, c in enumerate(p["dd"]))
    dyn = 17 + 3 * p["hclen"] + sum(p["cl_lens"][s] + CL_EXTRA.get(s, 0) for s, _ in p["hdr"])
    dyn += sum(c * (p["ll_lens"][s] + lext(s)) for s, c in enumerate(p["ll"])) + sum(c * (p["d_lens"][d] + _DEXT[d]) for d, c in enumerate(p["dd"]))
    return 5 + chunk_len + (0 if last else 5), fixed, dyn


def block_bytes(bits, last):
    """a block of `bits` bits and the trailer: the empty stored block behind a chunk that is not the last"""
    return (bits + (0 if last else 3) + 7) // 8 + (0 if last else 4)


def choice(tokens, chunk_len, last, flags=0, slot_cap=None):
    """-> "dynamic", "fixed" or "stored": what a level-2 task writes"""
    stored, fixed, dyn = sizes(tokens, chunk_len, last)
    cap = slot_bytes(chunk_len) if slot_cap is None else slot_cap
    if flags & ONLY_DYNAMIC:
        use = (block_bytes(dyn, last) + 3) // 4 * 4 <= cap
    else:
        use = dyn < fixed and (block_bytes(dyn, last) < stored or bool(flags & NO_STORED))
    if use:
        return "dynamic"
    return "stored" if block_bytes(fixed, last) >= stored and not flags & NO_STORED else "fixed"


class _Writer:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, k):
        """k bits, least significant first"""
        assert 0 <= value < (1 << k) or k == 0
        self.v |= value << self.n
        self.n += k

    def code(self, code, k):
        """a Huffman code of k bits, most significant first"""
        self.put(int(format(code, "0%db" % k)[::-1], 2) if k else 0, k)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def dynamic_block(tokens, last):
    """the exact bytes of a task that writes `tokens` as its dynamic block"""
    p = plan(tokens)
    llc, dc, clc = canonical(p["ll_lens"]), canonical(p["d_lens"]), canonical(p["cl_lens"])
    w = _Writer()
    w.put(int(bool(last)), 1)
    w.put(2, 2)
    w.put(p["hlit"] - 257, 5)
    w.put(p["hdist"] - 1, 5)
    w.put(p["hclen"] - 4, 4)
    for i in range(p["hclen"]):
        w.put(p["cl_lens"][CL_ORDER[i]], 3)
    for s, ex in p["hdr"]:
        w.code(clc[s], p["cl_lens"][s])
        w.put(ex, CL_EXTRA.get(s, 0))
    for t in tokens:
        if isinstance(t, tuple):
            s, eb, ex = len_symbol(t[0])
            w.code(llc[s], p["ll_lens"][s])
            w.put(ex, eb)
            d, eb, ex = dist_symbol(t[1])
            w.code(dc[d], p["d_lens"][d])
            w.put(ex, eb)
        else:
            w.code(llc[t], p["ll_lens"][t])
    w.code(llc[256], p["ll_lens"][256])
    assert w.n == sizes(tokens, 0, last)[2]
    if not last:
        w.put(0, 3)
        w.put(0, -w.n % 8)
        w.put(0xFFFF0000, 32)
    return w.bytes()


def _decoder(lens):
    """lengths -> {(length, code): symbol}"""
    return {(l, c): s for s, (l, c) in enumerate(zip(lens, canonical(lens))) if l}


def _symbol(b, table, top):
    c = 0
    for k in range(1, top + 1):
        c = (c << 1) | b.take(1)
        if (k, c) in table:
            return table[(k, c)]
    raise AssertionError("a code that the block's table does not have")


def _fixed_tables():
    ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    return _decoder(ll), _decoder([5] * 30)


def blocks(data):
    """the DEFLATE blocks in `data`, all three types ->
    [{"final", "btype", "bytes", "tokens", "matches", "end", "bits": the widest token's, and for btype 2 "ll_lens", "d_lens", "cl_lens", "hlit",
      "hdist", "hclen", "hdr"}]"""
    b = _Bits(data)
    out = []
    while b.n - b.at >= 3 and not (out and out[-1]["final"]):
        final, btype = b.take(1), b.take(2)
        assert btype in (0, 1, 2), btype
        blk = {"final": final, "btype": btype, "bytes": 0, "tokens": [], "matches": [], "bits": 0}
        if btype == 0:
            b.at = (b.at + 7) & ~7
            ln, nln = b.take(16), b.take(16)
            assert ln == (~nln & 0xFFFF)
            blk["tokens"] = list(b.d[b.at // 8: b.at // 8 + ln])
            b.skip(8 * ln)
            blk["bytes"] = ln
        else:
            if btype == 1:
                llt, dt = _fixed_tables()
            else:
                hlit, hdist, hclen = 257 + b.take(5), 1 + b.take(5), 4 + b.take(4)
                assert hlit <= 286 and hdist <= 30
                cl_lens = [0] * 19
                for i in range(hclen):
                    cl_lens[CL_ORDER[i]] = b.take(3)
                assert kraft(cl_lens, 7) == 1 << 7, "the code-length code is not complete"
                clt, lens, hdr = _decoder(cl_lens), [], []
                while len(lens) < hlit + hdist:
                    s = _symbol(b, clt, 7)
                    ex = b.take(CL_EXTRA.get(s, 0))
                    hdr.append((s, ex))
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        assert lens
                        lens += [lens[-1]] * (3 + ex)
                    else:
                        lens += [0] * ((3 if s == 17 else 11) + ex)
                assert len(lens) == hlit + hdist
                ll_lens, d_lens = lens[:hlit] + [0] * (286 - hlit), lens[hlit:] + [0] * (30 - hdist)
                assert kraft(ll_lens, 15) == 1 << 15 and kraft(d_lens, 15) == 1 << 15, "a code that is not complete"
                blk.update(ll_lens=ll_lens, d_lens=d_lens, cl_lens=cl_lens, hlit=hlit, hdist=hdist, hclen=hclen, hdr=hdr)
                llt, dt = _decoder(ll_lens), _decoder(d_lens)
            while True:
                at = b.at
                sym = _symbol(b, llt, 15)
                if sym == 256:
                    break
                if sym < 256:
                    blk["bytes"] += 1
                    blk["tokens"].append(sym)
                else:
                    assert sym <= 285
                    ln = _LBASE[sym - 257] + b.take(_LEXT[sym - 257])
                    dc = _symbol(b, dt, 15)
                    assert dc < 30
                    dist = _DBASE[dc] + b.take(_DEXT[dc])
                    assert 3 <= ln <= 258 and 1 <= dist <= 32768
                    blk["bytes"] += ln
                    blk["tokens"].append((ln, dist))
                    blk["matches"].append((ln, dist))
                blk["bits"] = max(blk["bits"], b.at - at)
        blk["end"] = b.at
        out.append(blk)
    assert b.n - b.at < 8 and (b.n == b.at or b.take(b.n - b.at) == 0), "bits behind the last block"
    return out


def tokens_of(data):
    """the tokens of a task's first block (Huffman), or None for a stored chunk"""
    blks = blocks(data)
    return blks[0]["tokens"] if blks[0]["btype"] else None


def expand(tokens, history=b""):
    """the bytes a token list stands for, behind `history`"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out[len(history):])
