"""CPU: the table-shape families (tests/table_shapes.py) before any kernel is involved -- the generator's
self-checks, the witnesses (oracle, plain-Python decode, zlib, the reference-made corpus_tables.json), the
geometry list against the sources, and the CENSUS: per table geometry, the decoded symbols of the families
take every route the geometry has, for literals, lengths, end-of-block and distances separately."""
import collections
import hashlib
import json
import os
import re
import zlib

import pytest

import table_shapes as ts
import token_fuzz as tf

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "debigulator_amd", "csrc")
GOLD = os.path.join(HERE, "golden")
ORC_UB_LONGCODE_500 = 0x40


@pytest.fixture(scope="module")
def families(oracle):
    fam = ts.families()
    for cs in fam.values():
        for c in cs:
            g, f, out, st = oracle.inflate(c.raw, c.cap, want_stats=True)
            c.exp, c.ub_flags = (g, f, out), st.ub_flags
    return fam


# ------------------------------------------------------------------ token_fuzz itself did not move
OLD_FAMILIES = {"F1": "dc2b5b7fd6690f8c", "F2": "de5f2d0b793552a6", "F3": "b6169377ac9de8bd", "F4": "d5ea925394b53caa",
                "F5": "d0ac2e74deed83a7", "F6": "3eb3588854bbf241", "F7": "4f7bef0b8aab0df0", "F8": "739eab6df0c479a8"}


def test_token_fuzz_families_are_byte_identical(oracle):
    """Stop tokens, max_len per case and the bit marks changed nothing for F1..F8: digests of (name, raw, recipient_size)
    taken before the change, and the reference-made fixture still holds the very streams golden_subset() makes"""
    fam = dict(tf.fixed_families())
    fam["F8"] = tf.f8_random(oracle.inflate)
    for name, cs in fam.items():
        h = hashlib.sha256()
        for c in cs:
            h.update(c.name.encode())
            h.update(c.raw)
            h.update(str(c.cap).encode())
        assert h.hexdigest()[:16] == OLD_FAMILIES[name], name
    items = json.load(open(os.path.join(GOLD, "corpus_tokens.json")))
    assert [(k["name"], k["raw_hex"], k["recipient_size"]) for k in items] == \
        [(c.name, c.raw.hex(), c.cap) for c in tf.golden_subset()]


# ------------------------------------------------------------------ the generator
def test_generator_self_checks(families):
    """every case has a defined answer from the reference (no ub flag but the named Q8 case's), none is skipped; the
    oracle and the plain-Python decode of the token list agree; sizes stay small"""
    assert {k: len(v) for k, v in families.items()} == {"T1": 14, "T2": 16, "T3": 9, "T4": 38, "T5": 20, "T6": 1130}
    flagged = {c.name: c.ub_flags for cs in families.values() for c in cs if c.ub_flags}
    assert flagged == {ts.Q8_CASE: ORC_UB_LONGCODE_500}
    longs = {c.name for c in ts.long_arms()}
    for name, cs in families.items():
        for c in cs:
            assert c.raw.endswith(tf.PAD) and len(c.raw) <= c.cap, c
            assert c.exp == (int(c.legal), len(c.plain), c.plain), c
            if c.name in longs:
                assert 40000 <= len(c.plain) <= 90000 and len(c.raw) > 4 * 1024, c
            elif name == "T6":
                assert len(c.raw) < 8000 and len(c.plain) < 70000, c
            else:
                assert len(c.plain) < 26000 and len(c.raw) < 1400, c
    assert all(c.legal for f in ts.COMPLETE for c in families[f])
    assert sum(not c.legal for c in families["T5"]) == 10


def test_zlib_decodes_every_complete_case(families):
    n = 0
    for f in ts.COMPLETE:
        for c in families[f]:
            z = zlib.decompressobj(-15)
            assert z.decompress(c.raw) == c.plain and z.eof and z.unused_data == tf.PAD, c
            n += 1
    assert n == 14 + 16 + 9 + 38 + 1130


def test_corpus_tables_is_the_golden_subset_and_the_oracle_agrees(oracle):
    """tests/golden/corpus_tables.json (tests/golden/make_golden.py: tables_corpus) holds the compiled reference's answers
    to golden_subset(): about 60 cases, at least 6 per family, every T3 and every T5 arm; the oracle gives the same"""
    items = json.load(open(os.path.join(GOLD, "corpus_tables.json")))
    sub = ts.golden_subset()
    assert [(k["name"], k["raw_hex"], k["recipient_size"]) for k in items] == [(c.name, c.raw.hex(), c.cap) for c in sub]
    per = collections.Counter(k["name"].split("/")[0] for k in items)
    assert 50 <= len(items) <= 70 and min(per.values()) >= 6 and set(per) == set(ts.families())
    assert os.path.getsize(os.path.join(GOLD, "corpus_tables.json")) <= 190 * 1024
    names = {k["name"] for k in items}
    assert all(c.name in names for c in ts.families()["T3"][:-1] + ts.families()["T5"])
    assert [k["name"] for k in items if k["oracle"] == "B" and k["good"]] == [ts.Q8_CASE]
    for k in items:
        g, f, out = oracle.inflate(bytes.fromhex(k["raw_hex"]), k["recipient_size"])
        assert (g, f, hashlib.sha256(out).hexdigest()) == (k["good"], k["final"], k["out_sha256"]), k["name"]


# ------------------------------------------------------------------ the geometry list against the sources
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _define(text, name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, text)
    assert m, f"{name} is no longer a plain #define: bring tests/table_shapes.py up to date"
    return int(m.group(1))


def test_geometry_list_matches_the_sources():
    """table_shapes.GEOMETRIES / STRUCT_GEOMETRY / SEG_BYTES / WIN_BYTES / ST_SEG_* restate facts of the .inc files; when
    one of these lines changes, the list -- and what the census proves -- is stale"""
    stale = "tests/table_shapes.py: the geometry list is stale -- "
    k, sp, st = _src("inflate_kernel.inc"), _src("inflate_split_kernel.inc"), _src("inflate_strand_kernel.inc")
    g10, g11 = ts.GEOMETRIES["g10"], ts.GEOMETRIES["g11"]
    assert (_define(k, "PB_LIT_1"), _define(k, "PB_LIT_MW"), _define(k, "PB_DIST")) == (g10.lit, g11.lit, g10.dist), stale + "PB_*"
    assert g10.dist == g11.dist
    assert "PBL = NW >= 2 ? PB_LIT_MW : PB_LIT_1;" in k, stale + "TabCfg"
    assert "CodeTabsT<TabCfg<NW>::PBL, uint32_t, (NW_ >= 2 ? %du : %du)> t;" % (g11.cap, g10.cap) in k, stale + "WaveLdsT"
    for text, struct in ((sp, "ScanLds"), (st, "StrandLds")):
        m = re.search(r"struct __attribute__\(\(aligned\(16\)\)\) %s \{(.*?)\n\};" % struct, text, re.S)
        assert m and "CodeTabsT<TabCfg<1>::PBL, uint16_t, %du> t;" % ts.GEOMETRIES[ts.STRUCT_GEOMETRY[struct]].cap in m.group(1), stale + struct
    assert "__shared__ ScanLds S;" in _src("inflate_chunk_kernel.inc"), stale + "chunk kernel"
    assert re.search(r"\n\s+StrandLds s;", _src("png_fused_kernel.inc")), stale + "fused PNG kernel"
    assert ts.STRUCT_GEOMETRY["chunk kernel"] == ts.STRUCT_GEOMETRY["ScanLds"]
    assert ts.STRUCT_GEOMETRY["fused PNG kernel"] == ts.STRUCT_GEOMETRY["StrandLds"]
    assert [ts.STRUCT_GEOMETRY[f"WaveLdsT<{n}>"] for n in (1, 2, 4, 8)] == ["g10", "g11", "g11", "g11"]
    assert re.findall(r"MAX_LINK_K = (\d+);", k) == [str(g11.max_k)], stale + "Fmt32::MAX_LINK_K"
    assert re.findall(r"MAX_LINK_K = (\d+);", sp) == [str(g10.max_k)], stale + "Fmt16::MAX_LINK_K"
    assert _define(k, "SEG_BYTES") == ts.SEG_BYTES and "WIN = 64u * NW * BYTES;" in k, stale + "SegCfg"
    assert "BYTES = NW >= 8 ? SEG_BYTES / 2 : SEG_BYTES;" in k and ts.WIN_BYTES == 64 * ts.SEG_BYTES, stale + "SegCfg"
    assert (int(re.search(r"#define ST_SEG_MIN (\d+)u", st).group(1)), int(re.search(r"#define ST_SEG_MAX (\d+)u", st).group(1))) == \
        (ts.ST_SEG_MIN, ts.ST_SEG_MAX), stale + "ST_SEG_*"
    import test_gpu_inflate  # the widths of the GPU suite, all of them mapped
    assert set(ts.WIDTH_GEOMETRY) == set(test_gpu_inflate.WIDTHS)
    assert all(set(v) <= set(ts.GEOMETRIES) for v in ts.WIDTH_GEOMETRY.values())


# ------------------------------------------------------------------ the census
def _census(families, g, only=None):
    """{(class, route): [case names]} over the decoded symbols; also per case the routes of its runs' first and last members"""
    cen, edges = collections.defaultdict(set), collections.defaultdict(set)
    for name, cs in families.items():
        if only and name not in only:
            continue
        for c in cs:
            cache = {}
            for bi, cls, s, bit, codes in ts.decoded_symbols(c):
                if cls == "stop":
                    continue
                if bi not in cache:
                    lit, dist, lruns, druns = ts.classify(codes[0], codes[1], g, want_runs=True)
                    cache[bi] = (lit, dist, {x[1][0] for x in lruns}, {x[1][-1] for x in lruns},
                                 {x[1][0] for x in druns}, {x[1][-1] for x in druns}, len(lruns), len(druns))
                lit, dist, lf, ll_, df, dl_, nl, nd = cache[bi]
                if cls == "dist":
                    r = dist[s]
                    edges[(c.name, bi, "dist")].add(("first", s) if s in df else None)
                    edges[(c.name, bi, "dist")].add(("last", s) if s in dl_ else None)
                else:
                    r = lit[s]
                    edges[(c.name, bi, "lit")].add(("first", s) if s in lf else None)
                    edges[(c.name, bi, "lit")].add(("last", s) if s in ll_ else None)
                cen[(cls, r)].add(c.name)
            for bi, v in cache.items():
                edges[(c.name, bi, "n")] = (v[6], v[7])
    return cen, edges


@pytest.mark.parametrize("gname", sorted(ts.GEOMETRIES))
def test_census_every_reachable_route_is_decoded(families, gname):
    """a condition on the generator, not a measurement: per geometry the decoded symbols include DIRECT, LINK(k) for
    every k the geometry has and -- where the geometry can reach it -- SLOW, for literals, length symbols, end-of-block
    and distance symbols separately, and never a symbol outside the probe range"""
    g = ts.GEOMETRIES[gname]
    cen, edges = _census(families, g)
    slow = [] if ts.unreachable(g) else [ts.SLOW]
    assert ts.unreachable(g) == (gname == "g11")  # the argument of the module docstring, for the geometry it is made for
    for cls in ("lit", "len", "eob"):
        want = [ts.DIRECT] + [ts.LINK(k) for k in range(1, 15 - g.lit + 1)] + slow
        assert {r for c, r in cen if c == cls} == set(want), (gname, cls)
    assert {r for c, r in cen if c == "dist"} == set([ts.DIRECT] + [ts.LINK(k) for k in range(1, 15 - g.dist + 1)] + slow)
    # T2: in every block, every run's first and last member is decoded
    for c in families["T2"]:
        for bi, codes in enumerate(c.codes):
            if codes is None:
                continue
            lit, dist, lruns, druns = ts.classify(codes[0], codes[1], g, want_runs=True)
            assert {("first", x[1][0]) for x in lruns} | {("last", x[1][-1]) for x in lruns} <= edges[(c.name, bi, "lit")]
            assert {("first", x[1][0]) for x in druns} | {("last", x[1][-1]) for x in druns} <= edges[(c.name, bi, "dist")]
    # ... and its own geometry's streams end a run at every length above the table, block b a distance run with k = b
    for c in families["T2"]:
        if c.name.split("/")[1] != gname or "/b" in c.name:
            continue
        dyn = [codes for codes in c.codes if codes is not None]
        assert len(dyn) == 6
        for b, codes in enumerate(dyn, 1):
            lit, dist, lruns, druns = ts.classify(codes[0], codes[1], g, want_runs=True)
            assert {r for r, _ in lruns} == {ts.LINK(k) for k in range(1, 15 - g.lit + 1)}, c
            assert [r for r, _ in druns] == [ts.LINK(b)], c
            if c.name.endswith("full"):  # (odd: a code of the next length may end end-of-block's run)
                assert lit[256] == (ts.LINK(b) if g.lit + b <= 15 else ts.DIRECT), c


def test_census_ladder_classes_at_every_long_length(families):
    """T1: the symbols its streams DECODE include a literal, a length symbol without extra bits, one with five extra bits
    and end-of-block at each code length 11, 12, 13, 14 and 15, and every block's two codes hold every length 1..15"""
    seen = set()
    for c in families["T1"]:
        for codes in c.codes:
            if codes is not None:
                assert {l for l in codes[0] if l} == {l for l in codes[1] if l} == set(range(1, 16)), c
        for bi, cls, s, bit, codes in ts.decoded_symbols(c):
            if cls == "lit":
                seen.add(("lit", codes[0][s]))
            elif cls == "eob":
                seen.add(("eob", codes[0][s]))
            elif cls == "len":
                seen.add(("len%d" % tf.LEN_EXTRA[s - 257], codes[0][s]))
    assert seen >= {(k, L) for k in ("lit", "len0", "len5", "eob") for L in range(11, 16)}, \
        sorted({(k, L) for k in ("lit", "len0", "len5", "eob") for L in range(11, 16)} - seen)


def test_census_capacity_arms(families):
    """T3 on the 10-bit / 256-entry geometry: the exact fit, the overflow by the smallest run, the literal side that
    starves the distance side and the one that leaves it exactly enough; the same streams hold no SLOW symbol and no
    full area behind the 11-bit tables, where the argument of table_shapes says none can"""
    g10, g11 = ts.GEOMETRIES["g10"], ts.GEOMETRIES["g11"]
    by = {c.name: c for c in families["T3"]}

    def shape(name, g):
        ll, dl = [x for x in by[name].codes if x is not None][0]
        lit, dist, lruns, druns = ts.classify(ll, dl, g, want_runs=True)
        return lit, dist, lruns, druns

    def entries(runs, pb, lens):
        return sum(1 << (lens[syms[-1]] - pb) for _, syms in runs)

    def lens_of(name):
        return [x for x in by[name].codes if x is not None][0]

    lit, dist, lruns, druns = shape("T3/exact/short", g10)
    assert entries(lruns, 10, lens_of("T3/exact/short")[0]) == 256 and ts.SLOW not in set(lit.values()) | set(dist.values())
    assert len(lruns) == 128 and {r for r, _ in lruns} == {ts.LINK(1)}
    for name in ("T3/over1/short", "T3/over1+eob/short"):
        lit, dist, lruns, druns = shape(name, g10)
        assert [r for r, _ in lruns] == [ts.LINK(1)] * 127 + [ts.SLOW] and len(lruns[-1][1]) == 4  # 254 + 4 = 258
    assert shape("T3/over1+eob/short", g10)[0][256] == ts.SLOW and shape("T3/over1/short", g10)[0][256] == ts.LINK(1)
    for name in ("T3/over2/short", "T3/over2+eob/ladder"):
        lit, dist, lruns, druns = shape(name, g10)
        ll = lens_of(name)[0]
        assert [r for r, _ in lruns] == [ts.LINK(1)] * 125 + [ts.LINK(2), ts.SLOW, ts.SLOW]
        assert [ll[s] for s in lruns[-3][1]] == [11, 12, 12] and entries(lruns[:-2], 10, ll) == 254
        assert [len(x[1]) for x in lruns[-2:]] == [4, 8]  # the run that overflows and the later one
    lit, dist, lruns, druns = shape("T3/over2+eob/ladder", g10)
    assert [r for r, _ in druns] == [ts.SLOW] and len(druns[0][1]) == 7 and lit[256] == ts.SLOW
    lit, dist, lruns, druns = shape("T3/exact/ladder", g10)
    assert ts.SLOW not in lit.values() and [r for r, _ in druns] == [ts.SLOW] and len(druns[0][1]) == 7
    lit, dist, lruns, druns = shape("T3/fit192/ladder", g10)
    assert entries(lruns, 10, lens_of("T3/fit192/ladder")[0]) == 192 and [r for r, _ in druns] == [ts.LINK(6)]
    assert ts.SLOW not in set(lit.values()) | set(dist.values())  # 192 + 64 = 256
    lit, dist, lruns, druns = shape("T3/miss194/ladder", g10)
    assert entries(lruns, 10, lens_of("T3/miss194/ladder")[0]) == 194 and [r for r, _ in druns] == [ts.SLOW]
    assert ts.SLOW not in lit.values()
    # every arm decodes symbols of its SLOW runs and of the last run that fits in the same block
    cen = collections.defaultdict(set)
    for c in families["T3"]:
        for bi, cls, s, bit, codes in ts.decoded_symbols(c):
            lit, dist = ts.classify(codes[0], codes[1], g10) if codes[1] is not None else (None, None)
            if lit is not None:
                cen[(c.name, bi)].add((dist if cls == "dist" else lit)[s])
    for name in by:
        if name.split("/")[1] not in ("exact", "fit192") or name == "T3/exact/ladder":
            assert any(ts.SLOW in v and (ts.LINK(1) in v or ts.LINK(2) in v) for k, v in cen.items() if k[0] == name), name
    # the 11-bit / 1024-entry geometry: unreachable, and these streams stay far from it
    assert ts.unreachable(g11) and not ts.unreachable(g10)
    for name in by:
        for codes in by[name].codes:
            if codes is not None:
                lit, dist, lruns, druns = ts.classify(codes[0], codes[1], g11, want_runs=True)
                assert ts.SLOW not in set(lit.values()) | set(dist.values())
                assert entries(lruns, 11, codes[0]) + entries(druns, 9, codes[1]) <= 628


def test_census_failing_tokens(families):
    """T5: the Stop of every `hit` case is the FIRST token that has no code inside the probe range, in both geometries;
    the `clean` cases decode the same code and never meet one; the Q7 arms' symbol lies outside [qmin, qmax] while a
    longer or equal probe range would hold it"""
    for c in families["T5"]:
        arm, hit = c.name.split("/", 1)[1].rsplit("/", 1)
        syms = ts.decoded_symbols(c)
        stops = [x for x in syms if x[1] == "stop"]
        assert len(stops) == (hit == "hit") and c.legal == (hit == "clean"), c
        for g in ts.GEOMETRIES.values():
            for bi, cls, s, bit, codes in syms:
                if cls == "stop":
                    lens = codes[1] if s.length is not None else codes[0]
                    assert s.nbits == 15 or arm.startswith("q7")
                    pat = (s.code << (15 - s.nbits)) | ((1 << (15 - s.nbits)) - 1)
                    assert not ts.has_code(lens, pat) and not ts.has_code(lens, pat & ~((1 << (15 - s.nbits)) - 1)), c
                    assert (cls, s) == syms[-1][1:3]  # nothing is decoded behind it
                    if arm.startswith("q7"):
                        sym = next(k for k, v in tf.canonical(lens).items() if v == s.code and lens[k] == s.nbits)
                        route = ts.classify(codes[0], codes[1], g)[1 if s.length is not None else 0][sym]
                        assert route == ts.OUT_OF_RANGE and lens[sym] > ts.probe_range(lens)[1], c
                else:
                    lit, dist = ts.classify(codes[0], codes[1], g) if codes[1] is not None else ts.classify(codes[0], None, g)
                    assert (dist if cls == "dist" else lit)[s] != ts.OUT_OF_RANGE, c
        if hit == "hit":
            assert c.exp[0] == 0 and 600 < c.exp[1] == len(c.plain), c  # good = 0, the final size at the partial count
        # Kraft sum below 1 for one of the two codes, never above it
        dyn = [codes for codes in c.codes if codes is not None][0]
        k = [sum(1 << (15 - l) for l in x if l) for x in dyn]
        assert all(v <= 32768 for v in k) and min(k) < 32768, c
    # where the unused pattern sits in the 10-bit geometry: a second-level entry, an empty direct slot, behind a SLOW mark
    g10 = ts.GEOMETRIES["g10"]
    where = {}
    for c in families["T5"]:
        if c.name.endswith("/hit") and "/q7/" not in c.name:
            ll, dl = [x for x in c.codes if x is not None][0]
            lit, dist, lruns, druns = ts.classify(ll, dl, g10, want_runs=True)
            runs = druns if c.name.startswith("T5/dist") else lruns
            where[c.name.split("/", 1)[1]] = runs[-1][0] if runs else ts.DIRECT
    assert where == {"lit/link/hit": ts.LINK(5), "dist/link/hit": ts.LINK(6), "lit/direct/hit": ts.DIRECT,
                     "dist/direct/hit": ts.DIRECT, "lit/slow/hit": ts.SLOW, "dist/slow/hit": ts.SLOW}


def test_census_block_pairs_reuse_slots_differently(families):
    """T4 behind the 10-bit tables: over the pairs of two dynamic blocks, the literal/length symbols the SECOND block decodes
    index direct-table slots that held something else in the first -- a link, a SLOW mark, another symbol, a slot beyond
    the second block's shrunken mask -- and its second-level runs lie on ranges the first block had cut differently: an
    entry left over from the first block would give other bytes, not the same ones"""
    g = ts.GEOMETRIES["g10"]
    seen = collections.Counter()
    kinds = set()
    for c in families["T4"]:
        dyn = [k for k, codes in enumerate(c.codes) if codes is not None]
        if "/pair/" not in c.name or len(dyn) != 2 or dyn[1] != dyn[0] + 1:
            continue
        kinds.add(c.name.split("/")[2])
        (l1, _), (l2, _) = c.codes[dyn[0]], c.codes[dyn[1]]
        s1, r1 = ts.direct_slots(l1, g.lit, g.cap, g.max_k)
        s2, r2 = ts.direct_slots(l2, g.lit, g.cap, g.max_k)
        used2 = {s for bi, cls, s, bit, codes in ts.decoded_symbols(c) if bi == dyn[1] and cls in ("lit", "len", "eob")}
        mine = {q: v for q, v in s2.items() if (v[0] == "D" and v[1] in used2) or v[0] != "D"}
        for q, v in mine.items():
            was = s1.get(q)
            if was is not None and was != v:
                seen[("former " + {"D": "symbol", "L": "link", "S": "SLOW"}[was[0]], v[0])] += 1
        if max(l2) < g.lit and max(l1) >= g.lit:
            seen["beyond the new mask"] += sum(q >= 1 << max(l2) for q in s1)
        cuts1 = {(b, n) for b, n, _ in r1}
        seen["old sub_tab range"] += sum(1 for b, n, syms in r2 if (b, n) not in cuts1 and any(b < b1 + n1 and b1 < b + n
                                                                                               for b1, n1 in cuts1))
    assert len(kinds) >= 16
    for was in ("former link", "former SLOW", "former symbol"):
        assert sum(v for k, v in seen.items() if isinstance(k, tuple) and k[0] == was) >= 1, (was, seen)
    assert seen["beyond the new mask"] >= 1 and seen["old sub_tab range"] >= 1, seen


def test_census_positions(families):
    """T1: the 48-bit token starts at every phase of a byte; T6: each probe group starts at every one of 1088 consecutive
    bit offsets (two scan segments), and the 48-bit token crosses the end of the staged window bit by 7 bits"""
    def tok48(c):
        k = -1
        for t in c.tokens:
            if not isinstance(t, ts.Block):
                k += 1
                if isinstance(t, tuple) and t[1] == 16385 + 8191 and tf.LEN_EXTRA[tf._LEN_SYM[t[0]][0]] == 5:
                    yield c.tok_bits[k], t
    ph = [next(tok48(c)) for c in families["T1"] if "/tok48/" in c.name]
    assert sorted(b % 8 for b, _ in ph) == list(range(8))
    for c in families["T1"]:
        if "/tok48/" in c.name:
            ll, dl = c.codes[1]
            bit, (n, d) = next(tok48(c))
            assert ll[257 + tf._LEN_SYM[n][0]] + 5 + dl[tf._dist_sym(d)[0]] + 13 == 48 and n - tf.LEN_BASE[tf._LEN_SYM[n][0]] == 31
    # T6: group starts = the token behind each run of fillers
    starts = collections.defaultdict(set)
    for c in families["T6"][:ts.T6_SPAN]:
        k, prev, grp = -1, None, -1
        for t in c.tokens:
            if isinstance(t, ts.Block):
                if t.kind == "dynamic":
                    grp += 1
                    armed = True
                continue
            k += 1
            if grp >= 0 and armed and t != 0:
                starts[grp].add(c.tok_bits[k])
                armed = False
    for grp in range(3):
        s = sorted(starts[grp])
        assert len(s) == ts.T6_SPAN >= 2 * 8 * ts.SEG_BYTES, grp
        assert {x % (8 * ts.SEG_BYTES) for x in s} == set(range(8 * ts.SEG_BYTES)), grp  # every offset inside a segment
    # the 15-bit end-of-block in front of a dynamic header, and the 15-bit literal in the stream's last bytes
    c = families["T6"][5]
    assert c.codes[1][0][256] == 15 and [kind for kind, _, _ in c.blocks] == ["fixed"] + ["dynamic"] * 3
    last = [t for t in c.tokens if not isinstance(t, ts.Block)][-1]
    assert c.codes[3][0][last] == 15 and c.n_bits - c.tok_bits[-1] == 15 + c.codes[3][0][256]
    # ... and the SLOW literal in front of the LINK literal
    lit, _ = ts.classify(c.codes[2][0], c.codes[2][1], ts.GEOMETRIES["g10"])
    grp2 = []
    seen = 0
    for t in c.tokens:
        if isinstance(t, ts.Block):
            seen += t.kind == "dynamic"
        elif seen == 2 and t != 0:
            grp2.append(lit[t])
    assert grp2[:2] == [ts.SLOW, ts.LINK(1)]
    # the window edge
    rel = []
    for c in families["T6"][ts.T6_SPAN:ts.T6_SPAN + len(ts.T6_EDGE)]:
        rel.append(next(tok48(c))[0] - c.blocks[1][1] - 8 * ts.WIN_BYTES)
    assert min(rel) <= -120 - 48 and max(rel) >= 0 and all(b - a == 7 for a, b in zip(rel, rel[1:])), rel
