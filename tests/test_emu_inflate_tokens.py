"""CPU: token-made DEFLATE streams (tests/token_fuzz.py) through the inflate kernels on the lock-step
emulator, every route, against the oracle.  The streams sit on the LZ77 edges that no encoder of the
suite reaches: distance 32 768 and 32 767 (TOK_MATCH's 15-bit field, hist_buf's reach, CK_HIST),
distance = bytes produced and one more on both sides of the first 32 KiB (chk_far), overlap around
the store widths, dependent chains, far matches into stored blocks across chunk tasks, 1032:1
expansion, matches that end on and cross recipient_size, and random token lists whose far distances
are as common as near ones.

Counts per route.  F1 60, F2 40, F3 36, F5 3, F7 80 streams on every route with skewed buffers.
The emulator is slow on the 2- / 4- / 8-wavefront, queued and pipe routes, so there F4 (6 streams) has
chains of 500 matches and F6 (4 streams) 500 matches instead of 2 000 and 4 000, and F8 is its first
30 streams (15 on the 8-wavefront route).  The one-wavefront, split, strand and chunked routes run the
full F4 and F6.  With skewed buffers the split, strand and 1024-byte chunked routes -- the three token
paths -- run all 300 streams of F8, the one-wavefront and 3072-byte chunked routes its first 60; with
aligned buffers all of them run its first 30.  With aligned buffers the five slow routes run every
third case of what they run with skewed ones (20, 14, 12, 2, 1, 2, 27 and 10 or 5 streams of F1..F8);
the other routes run every family in full there too."""
import hashlib
import json
import os
import zlib

import pytest

import emu_binding as eb
import token_fuzz as tf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ROUTES = [(1, {}), (2, {}), (4, {}), (8, {}), (eb.SPLIT, {}), (eb.SPLIT_QUEUED, {}), (eb.STRAND, {}),
          (eb.STRAND_PIPE, {}), (eb.CHUNKED, {"chunk_bytes": 1024}), (eb.CHUNKED, {"chunk_bytes": 3072})]
ROUTE_IDS = ["1", "2", "4", "8", "split", "queued", "strand", "pipe", "chunked1024", "chunked3072"]
THIN = (2, 4, 8, eb.SPLIT_QUEUED, eb.STRAND_PIPE)  # the routes on which the emulator is slow
F8_FULL = ((eb.SPLIT, 1024), (eb.STRAND, 1024), (eb.CHUNKED, 1024))  # (route, chunk_bytes) that run all of F8
MISALIGN = [(0, 0), (3, 5)]
FAMILIES = ["F1", "F2", "F3", "F4", "F5", "F6", "F7", "F8"]


@pytest.fixture(scope="module")
def emu():
    return eb.load_emu()


@pytest.fixture(scope="module")
def families(oracle):
    """every family once, with the oracle's answer beside each case; nothing changes them afterwards"""
    fam = dict(tf.fixed_families())
    fam["F4thin"] = tf.f4_dependent_chains(500)
    fam["F6thin"] = tf.f6_maximal_expansion(500)
    fam["F8"] = tf.f8_random(oracle.inflate)
    for cs in fam.values():
        for c in cs:
            g, f, out, st = oracle.inflate(c.raw, c.cap, want_stats=True)
            c.exp, c.ub_flags = (g, f, out), st.ub_flags
    return fam


def test_generator_emits_only_defined_streams(families):
    """a condition on the generator: the reference has a defined answer to every case"""
    for name, cs in families.items():
        assert [c.name for c in cs if c.ub_flags] == [], name
    assert [len(families[f]) for f in FAMILIES] == [60, 40, 36, 6, 3, 4, 80, 300]
    assert sum(c.damaged for c in families["F8"]) == 60
    assert all(2000 <= len(c.plain) <= 121000 for c in families["F8"])
    assert all(len(c.raw) <= c.cap for cs in families.values() for c in cs)  # Q1


def test_witnesses_agree(families):
    """before any kernel is involved: the oracle, the plain-Python decode of the token list and zlib
    say the same about every undamaged case; a distance one past the bytes produced makes zlib raise
    and the oracle stop with good = 0 and final = P (Q10); a match across recipient_size ends the
    oracle's decode in front of that match"""
    n_q10 = n_cross = 0
    for name, cs in families.items():
        for c in cs:
            if c.damaged:
                continue
            g, f, out = c.exp
            z = zlib.decompressobj(-15)
            if not c.legal:
                with pytest.raises(zlib.error):
                    z.decompress(c.raw)
                assert (g, f, out) == (0, len(c.plain), c.plain), c
                n_q10 += 1
                continue
            assert z.decompress(c.raw) == c.plain and z.eof and z.unused_data == tf.PAD, c
            if c.cap < len(c.plain):
                assert name == "F7" and (g, f, out) == (0, len(c.plain) - 258, c.plain[:-258]), c
                n_cross += 1
            else:
                assert (g, f, out) == (1, len(c.plain), c.plain), c
    assert n_q10 == 2 * 7 and n_cross == 2 * 8 * 3


def test_families_reach_the_edges_they_are_named_for(families):
    """what the case tables promise, counted on the token lists themselves"""
    def matches(c):
        pos = 0
        for t in c.tokens:
            if isinstance(t, tuple):
                yield pos, t[0], t[1]
                pos += t[0]
            elif not isinstance(t, tf.Block):
                pos += 1

    f1 = {(n, d) for c in families["F1"] for _, n, d in matches(c)}
    for code in range(30):
        for d in (tf.DIST_BASE[code], tf.DIST_BASE[code] + (1 << tf.DIST_EXTRA[code]) - 1):
            assert all((n, d) in f1 for n in tf.F1_LENGTHS)
    assert (258, 32768) in f1 and (257, 32768) in f1 and (3, 24577) in f1
    # F2: distance = position on the legal side, position + 1 on the other, and 32 768 behind 32 768
    last = {c.name: list(matches(c))[-1] for c in families["F2"]}
    for kind in ("fixed", "dynamic"):
        for P in tf.F2_P:
            assert last[f"F2/{kind}/P{P}/legal"][::2] == (P, P)
            assert P == 32768 or last[f"F2/{kind}/P{P}/q10"][::2] == (P, P + 1)
        for P in tf.F2_FAR_P:
            assert last[f"F2/{kind}/P{P}/far"][::2] == (P, 32768)
    # F4: 2 000 dependent matches per stream
    assert all(sum(1 for _ in matches(c)) >= 2000 for c in families["F4"])
    # F5: a dozen or more chunk tasks at both chunk sizes; a dozen of them open, in their first bytes, with a
    # match whose source starts exactly CK_HIST in front of it, in a stored block at least two blocks back
    for c in families["F5"]:
        by_pos = {pos: (n, d) for pos, n, d in matches(c)}

        def block_of(x):  # index of the block that produced output byte x
            return max(i for i, (_, _, pos) in enumerate(c.blocks) if pos <= x)

        for chunk in tf.F5_CHUNKS:
            starts = tf.f5_task_starts(c, chunk)
            far = [p for p in starts if by_pos.get(p, (0, 0))[1] == 32768]
            assert len(starts) >= 12 and len(far) >= 10, (c, chunk, len(starts), len(far))
            for p in far:
                n = by_pos[p][0]
                assert by_pos[p + n][1] == 32767
                src, dst = block_of(p - 32768), block_of(p)
                assert block_of(p - 32768 + n - 1) == src and c.blocks[src][0] == "stored"
                assert c.blocks[dst][0] == "dynamic" and c.blocks[dst][2] == p and dst - src >= 2
    # F6: 1032:1 -- 258 bytes for two bits
    d1 = families["F6"][0]
    assert len(d1.plain) == 1 + 4000 * 258 and len(d1.raw) < 4000 * 2 // 8 + 64
    # F8: distances are drawn per distance CODE, so the two top codes (above 16 384) are about as common as the
    # two lowest, less what the clipping to the bytes produced takes; some lie above what zlib can emit
    dist = [d for c in families["F8"] for _, _, d in matches(c)]
    assert len(dist) > 40000 and sum(d > 16384 for d in dist) > 2000 and sum(d > 32506 for d in dist) >= 20


def _select(families, fam, nw, kw, misalign):
    aligned, thin = misalign == (0, 0), nw in THIN
    if fam in ("F4", "F6"):
        cs = families[fam + "thin" if thin else fam]
    elif fam == "F8":
        if aligned or thin:
            cs = families["F8"][:15 if nw == 8 else 30]
        else:
            cs = families["F8"][:300 if (nw, kw.get("chunk_bytes", 1024)) in F8_FULL else 60]
    else:
        cs = families[fam]
    return cs[::3] if aligned and thin else cs


@pytest.mark.parametrize("misalign", MISALIGN, ids=["aligned", "skewed"])
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_every_route_agrees_with_the_oracle(emu, families, route, fam, misalign):
    nw, kw = route
    cs = _select(families, fam, nw, kw, misalign)
    outs, arena, offs = eb.emu_inflate(emu, [c.raw for c in cs], [c.cap for c in cs], nw=nw,
                                       in_misalign=misalign[0], out_misalign=misalign[1], **kw)
    for c, (good, final, out, r), (_, oo) in zip(cs, outs, offs):
        assert (good, final) == c.exp[:2], (c, r.status)
        assert out == c.exp[2], c
        # a match may overrun by 258 bytes: the fill behind the recipient is intact for 1 KiB
        assert (arena[oo + c.cap:oo + c.cap + 1024] == 0xA5).all(), c
    if nw == eb.CHUNKED and fam == "F5":
        # the chunk tasks themselves decoded them (at most one stream went to the one-kernel path)
        assert eb.last_split_retried <= 1


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_token_corpus_reference_made(emu, route):
    """tests/golden/corpus_tokens.json: the compiled reference's own answers to a subset of F1, F2, F3,
    F5 and F7, no oracle in between"""
    nw, kw = route
    items = json.load(open(os.path.join(GOLD, "corpus_tokens.json")))
    assert len(items) >= 36
    raws = [bytes.fromhex(k["raw_hex"]) for k in items]
    caps = [k["recipient_size"] for k in items]
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=nw, in_misalign=1, out_misalign=7, **kw)
    for k, (good, final, out, r) in zip(items, outs):
        assert (good, final, hashlib.sha256(out).hexdigest()) == (k["good"], k["final"], k["out_sha256"]), k["name"]
    for (io, oo), cap in zip(offs, caps):
        assert (arena[oo + cap:oo + cap + 1024] == 0xA5).all()
