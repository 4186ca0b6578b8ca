"""CPU: the table-shape families (tests/table_shapes.py) through the inflate kernels on the lock-step emulator, every
route emu_binding offers and the fused PNG kernel, bit for bit against the oracle -- which the fixture first holds to the
plain-Python decode of the token list; zlib and the census are tests/test_table_shapes_cpu.py's.

Thinning.  The one-wavefront, split, strand and chunked routes -- the four that are not in
test_emu_inflate_tokens.THIN -- run T1..T5 in full both ways and, with skewed buffers, ALL of T6: every one of the 1088
bit offsets, the window edge and the long arm on each route by itself (measured: 55..80 s per route on one core).
With aligned buffers they run T6's offsets 0..543 -- every bit offset of one scan segment, every phase of a byte --, every
window-edge stream and the long arm (30..35 s per route); the second segment is the skewed run's.  On the five
routes THIN names as slow T4 is every third pair (kinds i, j with i + j a multiple of 3) plus both six-block streams, and
T6 is every 48th offset, every 8th window-edge stream and the long arm (skewed), or every 96th and 16th (aligned).  T1,
T2, T3 and T5 -- every T3 and T5 arm -- run in full on every route both ways; test_thinning_floor holds the rule to that."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import emu_binding as eb
import png_spec_ref as R
import table_shapes as ts
import test_fused_png as tfp
from test_emu_inflate_tokens import THIN

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROUTES = [(1, {}), (2, {}), (4, {}), (8, {}), (eb.SPLIT, {}), (eb.SPLIT_QUEUED, {}), (eb.STRAND, {}),
          (eb.STRAND_PIPE, {}), (eb.CHUNKED, {"chunk_bytes": 1024})]
ROUTE_IDS = ["1", "2", "4", "8", "split", "queued", "strand", "pipe", "chunked1024"]
MISALIGN = [(0, 0), (3, 5)]
FAMILIES = ["T1", "T2", "T3", "T4", "T5", "T6"]
FAST = [nw for nw, _ in ROUTES if nw not in THIN]  # 1, split, strand, chunked


@pytest.fixture(scope="module")
def emu():
    L = eb.load_emu()
    L.emu_png_fused_batch.restype = C.c_int
    L.emu_png_fused_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)]
    L.emu_png_defilter_batch_w.restype = C.c_int
    L.emu_png_defilter_batch_w.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    return L


@pytest.fixture(scope="module")
def families(oracle):
    """every family once with the oracle's answer beside each case -- the witness's answer too, or the fixture fails"""
    fam = ts.families()
    for cs in fam.values():
        for c in cs:
            g, f, out, st = oracle.inflate(c.raw, c.cap, want_stats=True)
            assert (g, f, out) == (int(c.legal), len(c.plain), c.plain), c
            assert st.ub_flags == (0x40 if c.name == ts.Q8_CASE else 0), c
            c.exp, c.ub_flags = (g, f, out), st.ub_flags
    return fam


def _select(families, fam, nw, misalign):
    aligned, thin = misalign == (0, 0), nw in THIN
    cs = families[fam]
    if fam == "T4" and thin:
        return [c for p, c in enumerate(cs[:36]) if (p // 6 + p % 6) % 3 == 0] + cs[36:]
    if fam == "T6":
        main, edge, long = cs[:ts.T6_SPAN], cs[ts.T6_SPAN:-1], cs[-1:]
        if thin:
            return main[::96 if aligned else 48] + edge[::16 if aligned else 8] + long
        return main[:8 * ts.SEG_BYTES] + edge + long if aligned else cs
    return cs


def test_thinning_floor(families):
    for nw, _ in ROUTES:
        for mis in MISALIGN:
            for fam in ("T1", "T2", "T3", "T5"):
                assert _select(families, fam, nw, mis) == families[fam]
            t4 = _select(families, "T4", nw, mis)
            assert len(t4) >= 14 and {c.name for c in t4} >= {"T4/all6", "T4/all6rev"}
            # every kind still stands first and second in a pair
            firsts = {c.name.split("/")[2].split("-")[0] for c in t4 if "/pair/" in c.name}
            seconds = {c.name.split("/")[2].split("-")[1] for c in t4 if "/pair/" in c.name}
            assert firsts == seconds == set(ts.T4_KINDS)
            t6 = _select(families, "T6", nw, mis)
            assert len(t6) >= 12 + 3 + 1 and t6[-1].name == "T6/long" and any("edge" in c.name for c in t6)
    assert FAST == [1, eb.SPLIT, eb.STRAND, eb.CHUNKED]
    for nw in FAST:  # each of them by itself: nothing of T4 or T6 is left out with skewed buffers, one whole segment aligned
        assert _select(families, "T4", nw, (0, 0)) == _select(families, "T4", nw, (3, 5)) == families["T4"]
        assert _select(families, "T6", nw, (3, 5)) == families["T6"] and len(families["T6"]) == 1130
        names = [c.name for c in _select(families, "T6", nw, (0, 0))]
        assert names[:544] == [f"T6/off{k}" for k in range(544)] and len(names) == 544 + len(ts.T6_EDGE) + 1


@pytest.mark.parametrize("misalign", MISALIGN, ids=["aligned", "skewed"])
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_every_route_agrees_with_the_oracle(emu, families, route, fam, misalign):
    nw, kw = route
    cs = _select(families, fam, nw, misalign)
    outs, arena, offs = eb.emu_inflate(emu, [c.raw for c in cs], [c.cap for c in cs], nw=nw,
                                       in_misalign=misalign[0], out_misalign=misalign[1], **kw)
    for c, (good, final, out, r), (_, oo) in zip(cs, outs, offs):
        assert (good, final) == c.exp[:2], (c, r.status)
        assert out == c.exp[2], c
        assert (arena[oo + c.cap:oo + c.cap + 1024] == 0xA5).all(), c  # (the 32 bytes behind recipient_size among them)


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_tables_corpus_reference_made(emu, route):
    """tests/golden/corpus_tables.json: the compiled reference's own answers, no oracle in between"""
    nw, kw = route
    items = json.load(open(os.path.join(GOLD, "corpus_tables.json")))
    assert len(items) >= 60
    raws = [bytes.fromhex(k["raw_hex"]) for k in items]
    caps = [k["recipient_size"] for k in items]
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=nw, in_misalign=1, out_misalign=7, **kw)
    for k, (good, final, out, r) in zip(items, outs):
        assert (good, final, hashlib.sha256(out).hexdigest()) == (k["good"], k["final"], k["out_sha256"]), k["name"]
    for (io, oo), cap in zip(offs, caps):
        assert (arena[oo + cap:oo + cap + 1024] == 0xA5).all()


def test_fused_png_kernel_on_table_shapes(emu):
    """the PNG arm: T2, T3 and the six-block stream of T4 as one-row images through the fused inflate -> de-filter kernel
    (its StrandLds tables) and, inside tfp._run_both, through the unfused pair, field by field; the pixels against
    png_spec_ref.decode.  The fused kernel takes colour types 2, 3 and 6, so the row's bytes are indices into a grey
    palette here; tests/test_gpu_table_shapes.py decodes the same rows as 8-bit grey."""
    arm = ts.png_arm()
    pngs = [ts.png_file(raw, pixels, 3) for _, raw, pixels in arm]
    items = [tfp._split(p) for p in pngs]
    # four times the token workspace tfp._run_both takes by default: the six-block streams need 190..270 token rows, several
    # times what their input length is planned for (at the default size those five images go to the one-wavefront kernel)
    ws = 4 * (len(items) * (32 + 24576) + 12 * sum(len(it["raw"]) for it in items))
    out, retried = tfp._run_both(emu, items, ws_bytes=ws)
    for (name, _, pixels), png, (ig, pg, rgba) in zip(arm, pngs, out):
        st, px, _ = R.decode(png)
        assert st == 0 and ig == 1 and pg == 1, name
        assert np.array_equal(rgba, px.reshape(-1)), name
        assert bytes(px[0, :, 0]) == pixels and (px[0, :, 3] == 255).all(), name
    assert retried == 0  # every image is the fused kernel's own work


@pytest.mark.parametrize("nw", [1, 2, eb.SPLIT, eb.STRAND], ids=["1", "2", "split", "strand"])
def test_probe_counter_agrees_with_the_model(emu, families, nw):
    """the census from the other side: the emulator build counts the lengths huff_slow's canonical probe tries (the
    loop, not the link look-up).  A case whose tables hold no SLOW run by table_shapes.classify never enters the loop; a
    case that decodes SLOW symbols does; and behind the 11-bit / 1024-entry tables (two wavefronts) nothing ever does."""
    g = ts.GEOMETRIES["g11" if nw == 2 else "g10"]
    n_free = n_slow = 0
    for fam in ("T1", "T2", "T3", "T4", "T5"):
        for c in families[fam]:
            if c.name == "T3/long":
                continue
            marks = decoded = False
            for codes in c.codes:
                if codes is not None:
                    lit, dist = ts.classify(codes[0], codes[1], g)
                    marks |= ts.SLOW in set(lit.values()) | set(dist.values())
            for bi, cls, s, bit, codes in ts.decoded_symbols(c):
                if cls != "stop" and codes[1] is not None:
                    lit, dist = ts.classify(codes[0], codes[1], g)
                    decoded |= (dist if cls == "dist" else lit)[s] == ts.SLOW
            eb.slow_probes(emu)
            outs, _, _ = eb.emu_inflate(emu, [c.raw], [c.cap], nw=nw, in_misalign=1, out_misalign=2,
                                        ws_bytes=None if nw in (1, 2) else 4 << 20, no_handback=nw not in (1, 2))
            probes = eb.slow_probes(emu)
            assert outs[0][3].status != 11 and outs[0][:3] == c.exp, c  # the route's own kernel, no hand-back
            if not marks:
                assert probes == 0, c
                n_free += 1
            elif decoded:
                assert probes > 0, c
                n_slow += 1
    if nw == 2:
        assert n_slow == 0 and n_free == 14 + 16 + 8 + 38 + 20
    else:
        arms = {c.name for c in families["T3"] if c.name.split("/")[1].split("+")[0] in ("over1", "over2", "miss194")}
        assert n_slow >= len(arms) + 1 + 10 and n_free >= 14 + 16 + 2
