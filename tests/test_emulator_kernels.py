"""CPU: the product's HIP kernels compiled for the lock-step SIMT emulator
(tools/simt_emu) against the oracle / golden fixtures.  This exercises the very kernel
source that hipcc builds for gfx950 -- indexing, tiling, speculation, LZ77 resolve,
de-filter -- on machines without a GPU.  (The emulator says nothing about speed.)"""
import ctypes as C
import functools
import hashlib
import json
import os
import random
import zlib

import numpy as np
import pytest

import emu_binding as eb
from debigulator_amd import workload
from debigulator_amd._native import DebigPngImage, DebigPngResult

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    return eb.load_emu()


# wavefronts per stream: 1 = debig_inflate_kernel, 2 / 4 = debig_inflate_mw_kernel<NW>
@pytest.mark.parametrize("nw", [1, 2, 4, eb.SPLIT, eb.SPLIT_QUEUED, eb.STRAND, eb.STRAND_PIPE, eb.STRAND_PIPE_BIG])
def test_known_answers_and_corpus(emu, nw):
    items = json.load(open(os.path.join(GOLD, "kat.json")))
    items += json.load(open(os.path.join(GOLD, "corpus_zlib.json")))[:80 if nw in (1, eb.SPLIT, eb.SPLIT_QUEUED, eb.STRAND, eb.STRAND_PIPE, eb.STRAND_PIPE_BIG) else 40]
    raws = [bytes.fromhex(k["raw_hex"]) for k in items]
    caps = [k["recipient_size"] for k in items]
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=nw, in_misalign=3, out_misalign=5)
    for k, (good, final, out, r) in zip(items, outs):
        assert good == k["good"] and final == k["final"], k.get("name")
        want = k.get("out_hex")
        if want is not None:
            assert out.hex() == want
        else:
            assert hashlib.sha256(out).hexdigest() == k["out_sha256"]
    for (io, oo), cap in zip(offs, caps):  # guard bytes behind every recipient are intact
        assert (arena[oo + cap:oo + cap + 32] == 0xA5).all()


@pytest.mark.parametrize("nw", [1, 4, eb.SPLIT, eb.SPLIT_QUEUED, eb.STRAND, eb.STRAND_PIPE, eb.STRAND_PIPE_BIG])
def test_corrupt_corpus_reference_made(emu, nw):
    """tests/golden/corpus_corrupt.json: damaged streams with the REFERENCE's own answers (build B)"""
    items = json.load(open(os.path.join(GOLD, "corpus_corrupt.json")))[:: 1 if nw in (1, eb.SPLIT, eb.SPLIT_QUEUED, eb.STRAND, eb.STRAND_PIPE, eb.STRAND_PIPE_BIG) else 3]
    raws = [bytes.fromhex(k["raw_hex"]) for k in items]
    caps = [k["recipient_size"] for k in items]
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=nw, out_misalign=1)
    for k, (good, final, out, r) in zip(items, outs):
        assert (good, final, hashlib.sha256(out).hexdigest()) == (k["good"], k["final"], k["out_sha256"])
    for (io, oo), cap in zip(offs, caps):
        assert (arena[oo + cap:oo + cap + 32] == 0xA5).all()


@pytest.mark.parametrize("nw", [1, eb.SPLIT, eb.STRAND])
@pytest.mark.parametrize("kind", ["stored", "fixed", "dynamic"])
def test_cfg2_streams(emu, oracle, kind, nw):
    pairs = workload.make_streams(kind, 3, 65536)
    raws = [p[0] for p in pairs]
    caps = [max(65537, len(r)) for r in raws]
    outs, _, _ = eb.emu_inflate(emu, raws, caps, nw=nw)
    if nw in (eb.SPLIT, eb.STRAND):
        assert eb.last_split_retried == 0  # the scan / LZ77 pair itself decoded them
    for (good, final, out, r), (raw, plain) in zip(outs, pairs):
        assert (good, final) == (1, 65536) and out == plain.tobytes()
        if kind != "stored":
            assert r.n_windows > 0 and r.n_rounds / r.n_windows < 6  # speculation converges fast


def test_eight_wavefront_kernel_with_half_size_segments(emu, oracle):
    """debig_inflate_mw_kernel<8>: 512 threads, 34-byte segments, round 0 starting one segment
    early.  A dynamic stream that crosses windows and the 32 KiB tile, plus damaged streams."""
    raw, plain = workload.make_stream("dynamic", 9, 98304)
    rng = random.Random(8)
    raws, caps = [raw], [98305]
    for it in range(8):
        data = bytes(rng.choice(b"abcdefgh \n") for _ in range(rng.randint(100, 5000)))
        r = bytearray(zlib.compress(data, 6)[2:-4])
        if it % 2:
            r[rng.randrange(len(r))] ^= 1 << rng.randrange(8)
        raws.append(bytes(r))
        caps.append(len(data) * 3 + 64)
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=8, out_misalign=7)
    assert (outs[0][0], outs[0][1]) == (1, 98304) and outs[0][2] == plain.tobytes()
    for raw_i, cap, (good, final, out, r) in zip(raws[1:], caps[1:], outs[1:]):
        eg, ef, eo, st = oracle.inflate(raw_i, cap, want_stats=True)
        if st.ub_flags & (0x10 | 0x02):
            continue
        assert (good, final, out) == (eg, ef, eo)


def test_multi_wavefront_kernel_crosses_windows_and_tiles(emu):
    """One 64 KiB dynamic-Huffman stream through the 4-wavefront kernel: several 17 KiB input
    windows, the 16 KiB output tile rolls over, matches are resolved by all wavefronts."""
    raw, plain = workload.make_stream("dynamic", 5, 65536)
    outs, _, _ = eb.emu_inflate(emu, [raw], [65537], nw=4, out_misalign=9)
    good, final, out, r = outs[0]
    assert (good, final) == (1, 65536) and out == plain.tobytes()
    assert r.n_windows >= 2


@pytest.mark.parametrize("nw", [1, 4, eb.SPLIT, eb.STRAND, eb.STRAND_PIPE])
def test_end_position_and_no_gates_flag(emu, nw):
    """debig_result.in_end_bits (where decoding stopped) and DEBIG_STREAM_NO_REF_GATES: what a
    container with several members needs (debig_gunzip_batch).  A raw stream followed by other
    bytes is decoded with in_len covering all of them; the reported end is the last bit of the
    DEFLATE data, and the reference's size gates (Q1) do not apply."""
    rng = random.Random(12)
    raws, plains, ends = [], [], []
    for it in range(12):
        data = bytes(rng.choice(b"abcdefgh \n") for _ in range(rng.randint(1, 9000)))
        strat = rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY])
        c = zlib.compressobj(rng.choice([0, 1, 9]), zlib.DEFLATED, -15, 9, strat)
        raw = c.compress(data) + c.flush()
        tail = bytes(rng.getrandbits(8) for _ in range(rng.randint(8, 40)))
        raws.append(raw + tail)
        plains.append(data)
        ends.append(len(raw))
    caps = [len(p) for p in plains]  # exact: smaller than in_len for the short ones (gate Q1 would reject)
    outs, _, _ = eb.emu_inflate(emu, raws, caps, nw=nw, flags=1)
    for (good, final, out, r), plain, end in zip(outs, plains, ends):
        assert (good, final, out) == (1, len(plain), plain)
        assert (r.in_end_bits + 7) // 8 == end
    # without the flag the same descriptors hit the reference's gate when recipient < input
    outs, _, _ = eb.emu_inflate(emu, raws, caps, nw=nw)
    assert any(good == 0 and r.status == 1 for good, _, _, r in outs)


def _tiny_block_streams(seed, count, max_len):
    """Streams whose encoder flushed every few bytes (what PNG writers that flush per row
    produce, e.g. extraturns.png: 801 blocks for 640 KB): hundreds of blocks of a few bytes,
    fixed and dynamic codes, empty stored blocks in between; a third damaged."""
    rng = random.Random(seed)
    raws, caps = [], []
    for it in range(count):
        data = bytes(rng.choice(b"abcdefgh \n") for _ in range(rng.randint(20, max_len)))
        strat = rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY])
        c = zlib.compressobj(rng.choice([1, 6, 9]), zlib.DEFLATED, -15, 9, strat)
        raw, i, maxchunk = b"", 0, rng.choice([3, 20, 60, 200])
        while i < len(data):
            n = rng.randint(1, maxchunk)
            raw += c.compress(data[i:i + n])
            i += n
            raw += c.flush(rng.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_BLOCK]))
        raw = bytearray(raw + c.flush())
        mode = it % 3
        if mode == 1:
            raw = raw[: rng.randint(5, len(raw))]
        elif mode == 2:
            raw[rng.randrange(len(raw))] ^= 1 << rng.randrange(8)
        raws.append(bytes(raw))
        caps.append(max(len(data) * 3 + 64, len(raw)))
    return raws, caps


@pytest.mark.parametrize("nw", [1, 4, eb.SPLIT, eb.STRAND, eb.STRAND_PIPE])
def test_streams_of_tiny_blocks_take_the_probe_path(emu, oracle, nw):
    raws, caps = _tiny_block_streams(31 + nw, 12 if nw == 1 else 6, 1500)
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=nw, in_misalign=5, out_misalign=11)
    probed = 0
    for raw, cap, (good, final, out, r), (_, oo) in zip(raws, caps, outs, offs):
        eg, ef, eo, st = oracle.inflate(raw, cap, want_stats=True)
        assert (arena[oo + cap:oo + cap + 32] == 0xA5).all()
        if st.ub_flags & (0x10 | 0x02):
            continue
        assert (good, final, out) == (eg, ef, eo)
        probed += r.n_windows > 8 and r.n_rounds < 2 * r.n_windows  # one probe instead of >= 2 rounds
    assert probed >= 2


def test_mixed_width_launches_partition_the_batch(emu, oracle):
    """debig_hip_inflate_batch_ex's mixed mode: the 4-wavefront kernel takes the large class
    (>= 256 KiB input or >= 1 MiB recipient), the 1-wavefront kernel the rest; together they
    decode every stream exactly once."""
    rng = random.Random(9)
    raws, caps = [], []
    for it in range(10):
        data = bytes(rng.choice(b"abcdefgh ") for _ in range(rng.randint(100, 6000)))
        raws.append(zlib.compress(data, 6)[2:-4])
        caps.append((1 << 20) + it if it % 2 else len(data) + 7)  # odd ones are "large" by recipient
    exp = [oracle.inflate(r, c) for r, c in zip(raws, caps)]
    outs, _, _ = eb.emu_inflate(emu, raws, caps, classes=[(4, 2), (1, 1)])
    assert [(g, f, o) for g, f, o, _ in outs] == [tuple(e) for e in exp]
    only_large, _, _ = eb.emu_inflate(emu, raws, caps, classes=[(4, 2)])
    assert [r.final_set for _, _, _, r in only_large] == [it % 2 for it in range(10)]


@pytest.mark.parametrize("nw", [1, 4, eb.SPLIT, eb.STRAND, eb.STRAND_PIPE])
def test_corrupt_streams_agree_with_oracle(emu, oracle, nw):
    rng = random.Random(4)
    raws, caps = [], []
    for it in range(60 if nw == 1 else 30):
        data = bytes(rng.choice(b"abcdefgh ") for _ in range(rng.randint(50, 3000)))
        raw = bytearray(zlib.compress(data, rng.choice([1, 6, 9]))[2:-4])
        if rng.random() < 0.5:
            raw = raw[: rng.randint(5, len(raw))]
        else:
            raw[rng.randrange(len(raw))] ^= 1 << rng.randrange(8)
        raws.append(bytes(raw))
        caps.append(len(data) * 4 + 64)
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=nw)
    for raw, cap, (good, final, out, r) in zip(raws, caps, outs):
        eg, ef, eo, st = oracle.inflate(raw, cap, want_stats=True)
        if st.ub_flags & (0x10 | 0x02):
            continue
        assert (good, final, out) == (eg, ef, eo)


@pytest.mark.parametrize("nw", [1, 4, eb.SPLIT, eb.STRAND, eb.STRAND_PIPE, eb.STRAND_PIPE_BIG])
def test_p2_aliasing_replay_matches_reference_digest(emu, nw):
    """phoebus.png: the inflate kernel with the decode_png aliasing parameters + the
    de-filter kernel reproduce the reference's (corrupted-tail) output."""
    gold = json.load(open(os.path.join(GOLD, "resources.json")))["png"]["phoebus.png"]
    data = open(os.path.join(GOLD, "resources", "phoebus.png"), "rb").read()
    w, h = gold["width"], gold["height"]
    # host-side container walk (same rules as csrc/host/debig_png.c), in python for the test
    at, z = 8, b""
    while at + 8 <= len(data):
        ln = int.from_bytes(data[at:at + 4], "big")
        if data[at + 4:at + 8] == b"IDAT":
            z += data[at + 8:at + 8 + ln]
        at += 12 + ln
    raw = z[2:-4]
    est = 4 * w * h + h + 1
    s0 = est - 772 + ((16 - (est & 15)) & 15)
    outs, arena, offs = eb.emu_inflate(emu, [raw], [est], nw=nw, p2=[(s0, est)])
    good, final, stream, r = outs[0]
    assert good == 1 and final == est - 1
    rgba = _emu_defilter(emu, stream, w, h, 6)
    assert hashlib.sha256(rgba.tobytes()).hexdigest() == gold["rgba_sha256"]


def _emu_defilter(emu, stream, w, h, ct, palette=None, nwd=1, expect_good=1):
    emu.emu_png_defilter_batch_w.restype = C.c_int
    emu.emu_png_defilter_batch_w.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    sa = np.zeros(len(stream) + 1024 + 768, dtype=np.uint8)
    sa[1:1 + len(stream)] = np.frombuffer(stream, dtype=np.uint8)  # odd offset: rows are never aligned
    pal_off = (1 + len(stream) + 15) // 16 * 16
    if palette is not None:
        sa[pal_off:pal_off + 768] = palette
    rgba = np.zeros(4 * w * h + 64, dtype=np.uint8)
    img = (DebigPngImage * 1)()
    img[0].stream_off, img[0].rgba_off, img[0].pal_off = 1, 0, pal_off
    img[0].width, img[0].height, img[0].color_type, img[0].asserts_off = w, h, ct, 0
    res = (DebigPngResult * 1)()
    assert emu.emu_png_defilter_batch_w(sa.ctypes.data, rgba.ctypes.data, img, res, 1, nwd) == 0
    assert res[0].good == expect_good
    if not expect_good:
        return res[0].bad_row
    return rgba[: 4 * w * h]


def test_defilter_kernel_all_filter_types(emu, oracle):
    for p in json.load(open(os.path.join(GOLD, "png_synth.json"))):
        if not p["good"]:
            # the stored-block 33x7 image: its DEFLATE stream is LONGER than the recipient the
            # reference hands to inflate (est = 4wh+h+1), so the reference's own gate
            # recipient_size < compressed_input_size rejects a valid PNG (Q1)
            continue
        png = bytes.fromhex(p["png_hex"])
        at, z, plte = 8, b"", None
        while at + 8 <= len(png):
            ln = int.from_bytes(png[at:at + 4], "big")
            typ = png[at + 4:at + 8]
            if typ == b"IDAT":
                z += png[at + 8:at + 8 + ln]
            if typ == b"PLTE":
                plte = np.frombuffer(png[at + 8:at + 8 + ln], dtype=np.uint8).reshape(-1, 3)
            at += 12 + ln
        stream = zlib.decompress(z)
        pal = None
        if plte is not None:
            pal = np.zeros(768, dtype=np.uint8)
            pal[0:len(plte)] = plte[:, 0]
            pal[256:256 + len(plte)] = plte[:, 1]
            pal[512:512 + len(plte)] = plte[:, 2]
        rgba = _emu_defilter(emu, stream, p["w"], p["h"], p["ct"], pal)
        assert hashlib.sha256(rgba.tobytes()).hexdigest() == p["rgba_sha256"], (p["w"], p["h"], p["ct"], p["ftype"])


def _spec_defilter(stream, w, h, bpp):
    """PNG specification de-filter (what src/decode_png.c:1430-1507 computes for bpp 4 and 1),
    written independently of the kernel: bytes of the de-filtered rows, [h, w*bpp]."""
    rowb = w * bpp
    out = np.zeros((h, rowb), dtype=np.uint8)
    for y in range(h):
        ft = stream[y * (rowb + 1)]
        line = stream[y * (rowb + 1) + 1:(y + 1) * (rowb + 1)]
        for i in range(rowb):
            a = int(out[y, i - bpp]) if i >= bpp else 0
            b = int(out[y - 1, i]) if y > 0 else 0
            c = int(out[y - 1, i - bpp]) if (y > 0 and i >= bpp) else 0
            if ft == 0:
                pr = 0
            elif ft == 1:
                pr = a
            elif ft == 2:
                pr = b
            elif ft == 3:
                pr = (a + b) >> 1
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                pr = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            out[y, i] = (int(line[i]) + pr) & 0xFF
    return out


@pytest.mark.parametrize("ct", [6, 3, 2])
def test_defilter_kernel_group_and_band_edges(emu, ct):
    """Widths around the 4-pixel group (partial last group, rows shorter than a group) and
    heights around the 64-row band, filter type chosen per row at random.  Colour type 2 runs
    the spec-conforming expansion here (replay_p3 = 0; the reference's own output for RGB is
    test_p3_rgb_replay_kernel_matches_reference_digest)."""
    rng = np.random.default_rng(100 + ct)
    bpp = {6: 4, 3: 1, 2: 3}[ct]
    pal = rng.integers(0, 256, 768, dtype=np.uint8) if ct == 3 else None
    for w, h in [(1, 1), (2, 3), (3, 65), (4, 64), (5, 2), (7, 130), (8, 63), (63, 5), (65, 66), (130, 9)]:
        stream = rng.integers(0, 256, h * (w * bpp + 1), dtype=np.uint8)
        stream[:: w * bpp + 1] = rng.integers(0, 5, h)
        want = _spec_defilter(stream, w, h, bpp).reshape(h, w, bpp)
        rgba = _emu_defilter(emu, stream.tobytes(), w, h, ct, pal).reshape(h, w, 4)
        if ct == 6:
            exp = want
        elif ct == 2:
            exp = np.concatenate([want, np.full((h, w, 1), 255, np.uint8)], axis=2)
        else:
            idx = want[:, :, 0].astype(np.int64)
            exp = np.stack([pal[idx], pal[256 + idx], pal[512 + idx], np.full((h, w), 255, np.uint8)], axis=2)
        assert np.array_equal(rgba, exp), (ct, w, h)


@pytest.mark.parametrize("nwd", [2, 4, 8, 16])
def test_defilter_kernel_several_wavefronts_per_image(emu, nwd):
    """debig_png_defilter_kernel<NWD>: the bands of one image pipelined through NWD wavefronts (band
    k+1 runs about 80 groups behind band k and takes the row above it from the output).  Images
    with more bands than wavefronts, rows shorter and longer than the pipeline distance, a palette
    image (stays on one wavefront), and a bad filter byte in a late band (fails the image with
    the first bad row, whichever wavefront meets it)."""
    rng = np.random.default_rng(500 + nwd)
    for ct, w, h in [(6, 3, 200), (6, 70, 130), (6, 700, 64 * nwd + 70), (2, 90, 64 * nwd + 3), (6, 1300, 129), (3, 50, 200)]:
        bpp = {6: 4, 3: 1, 2: 3}[ct]
        pal = rng.integers(0, 256, 768, dtype=np.uint8) if ct == 3 else None
        stream = rng.integers(0, 256, h * (w * bpp + 1), dtype=np.uint8)
        stream[:: w * bpp + 1] = rng.integers(0, 5, h)
        want = _spec_defilter(stream, w, h, bpp).reshape(h, w, bpp)
        rgba = _emu_defilter(emu, stream.tobytes(), w, h, ct, pal, nwd=nwd).reshape(h, w, 4)
        if ct == 6:
            exp = want
        elif ct == 2:
            exp = np.concatenate([want, np.full((h, w, 1), 255, np.uint8)], axis=2)
        else:
            idx = want[:, :, 0].astype(np.int64)
            exp = np.stack([pal[idx], pal[256 + idx], pal[512 + idx], np.full((h, w), 255, np.uint8)], axis=2)
        assert np.array_equal(rgba, exp), (ct, w, h, nwd)
    w, h = 40, 64 * nwd + 100
    stream = rng.integers(0, 256, h * (w * 4 + 1), dtype=np.uint8)
    stream[:: w * 4 + 1] = rng.integers(0, 5, h)
    for bad in (64 * nwd + 17, 70):
        stream[bad * (w * 4 + 1)] = 9
    assert _emu_defilter(emu, stream.tobytes(), w, h, 6, nwd=nwd, expect_good=0) == 70


def test_defilter_workgroups_of_an_image_never_resident_together(emu):
    """The several-workgroups-per-image de-filter (debig_png_defilter_kernel<4, 16, true>) needs an image's
    workgroups resident together; when they are not (fewer CUs than assumed, another stream's kernels holding
    LDS -- here: the emulator, which runs ONE workgroup at a time) a workgroup that waits in vain gives the
    image up as REDO, never as bad (src/decode_png.c:1430-1507 does not fail a valid image), and the
    one-workgroup pass that follows decodes exactly those images: the pixels are the specification's, a row
    with a bad filter byte still fails its image with the first bad row."""
    emu.emu_png_defilter_mwg.restype = C.c_int
    emu.emu_png_defilter_mwg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_uint32)]
    rng = np.random.default_rng(77)
    shapes = [(6, 120, 64 * 17 + 5, None), (2, 90, 64 * 18 + 3, None), (6, 40, 700, 650), (6, 33, 40, None)]
    n = len(shapes)
    streams, exps = [], []
    for ct, w, h, bad in shapes:
        bpp = {6: 4, 2: 3}[ct]
        st = rng.integers(0, 256, h * (w * bpp + 1), dtype=np.uint8)
        st[:: w * bpp + 1] = rng.integers(0, 5, h)
        want = _spec_defilter(st, w, h, bpp).reshape(h, w, bpp)
        if ct == 2:
            want = np.concatenate([want, np.full((h, w, 1), 255, np.uint8)], axis=2)
        if bad is not None:
            st[bad * (w * bpp + 1)] = 7
        streams.append(st)
        exps.append(want)
    sa = np.zeros(sum(len(s) + 32 for s in streams) + 1024, dtype=np.uint8)
    rgba = np.zeros(sum(4 * w * h + 64 for _, w, h, _ in shapes), dtype=np.uint8)
    img = (DebigPngImage * n)()
    res = (DebigPngResult * n)()
    so, ro = 3, 0
    for i, ((ct, w, h, bad), st) in enumerate(zip(shapes, streams)):
        sa[so:so + len(st)] = st
        img[i].stream_off, img[i].rgba_off, img[i].pal_off = so, ro, 0
        img[i].width, img[i].height, img[i].color_type, img[i].asserts_off = w, h, ct, 0
        so += len(st) + 29
        ro += 4 * w * h + 64
    n_redo = C.c_uint32(0)
    assert emu.emu_png_defilter_mwg(sa.ctypes.data, rgba.ctypes.data, img, res, n, 4, C.byref(n_redo)) == 0
    assert n_redo.value >= 2  # the images with more bands than the image's 16 wavefronts (the ring wraps: a workgroup run earlier
    # waits for one that has not started) were given up first ...
    for i, ((ct, w, h, bad), want) in enumerate(zip(shapes, exps)):
        if bad is not None:  # ... a real bad row is still a failed image
            assert (res[i].good, res[i].bad_row) == (0, bad)
            continue
        assert res[i].good == 1, i  # ... and came back as the specification's pixels
        got = rgba[img[i].rgba_off: img[i].rgba_off + 4 * w * h].reshape(h, w, 4)
        assert np.array_equal(got, want), i


def test_defilter_pixel_skew_step_one_workgroup(emu):
    """debig_png_defilter_kernel<4, 16, true, true> ("PX": a lane runs one PIXEL behind the row above, the "up" pixels of a
    macro-step come from the lane above in the same macro-step) with ONE workgroup per image, i.e. no wait across
    workgroups: RGBA images of odd widths and heights (narrower than a wavefront's skew, one pixel wide, many bands),
    every filter type per row, against the PNG specification's pixels; an RGB image beside them takes the group step."""
    emu.emu_png_defilter_mwg.restype = C.c_int
    emu.emu_png_defilter_mwg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.c_uint32)]
    rng = np.random.default_rng(4242)
    shapes = [(6, 301, 64 * 5 + 9), (6, 1, 70), (6, 2, 300), (6, 3, 5), (6, 64, 64), (6, 67, 129), (2, 90, 64 * 4 + 3),
              (6, 1030, 66), (6, 5, 64 * 9 + 1)]
    n = len(shapes)
    streams, exps = [], []
    for k, (ct, w, h) in enumerate(shapes):
        bpp = {6: 4, 2: 3}[ct]
        st = rng.integers(0, 256, h * (w * bpp + 1), dtype=np.uint8)
        st[:: w * bpp + 1] = rng.integers(0, 5, h)
        if k in (0, 4, 5):  # bands whose rows are ALL Paeth take the step without predictor selects (k = 0: all but one band)
            st[:: w * bpp + 1] = 4
            if k == 0:
                st[70 * (w * bpp + 1)] = 3
        want = _spec_defilter(st, w, h, bpp).reshape(h, w, bpp)
        if ct == 2:
            want = np.concatenate([want, np.full((h, w, 1), 255, np.uint8)], axis=2)
        streams.append(st)
        exps.append(want)
    sa = np.zeros(sum(len(s) + 32 for s in streams) + 1024, dtype=np.uint8)
    rgba = np.zeros(sum(4 * w * h + 64 for _, w, h in shapes), dtype=np.uint8)
    img = (DebigPngImage * n)()
    res = (DebigPngResult * n)()
    so, ro = 1, 0
    for i, ((ct, w, h), st) in enumerate(zip(shapes, streams)):
        sa[so:so + len(st)] = st
        img[i].stream_off, img[i].rgba_off, img[i].pal_off = so, ro, 0
        img[i].width, img[i].height, img[i].color_type, img[i].asserts_off = w, h, ct, 0
        so += len(st) + 30 + (i & 3)
        ro += 4 * w * h + 64
    n_redo = C.c_uint32(0)
    assert emu.emu_png_defilter_mwg(sa.ctypes.data, rgba.ctypes.data, img, res, n, 1, C.byref(n_redo)) == 0
    assert n_redo.value == 0
    for i, ((ct, w, h), want) in enumerate(zip(shapes, exps)):
        assert res[i].good == 1, i
        got = rgba[img[i].rgba_off: img[i].rgba_off + 4 * w * h].reshape(h, w, 4)
        assert np.array_equal(got, want), (i, shapes[i])


def test_p3_rgb_replay_kernel_matches_reference_digest(emu):
    """colour type 2 through debig_png_p3_kernel on the emulator: a small synthetic RGB image
    against the oracle (pinned to the reference on this behaviour by backgrounddetailed1.png)."""
    from oracle.binding import Oracle

    orc = Oracle()
    png, _ = workload.make_png(4242, 37, 21, ct=2, ftype=5, noise=9, enc="dynamic", idat_chunk=4096)
    prior = (np.arange(37 * 21 * 4, dtype=np.uint32) * 40503 >> 7).astype(np.uint8)
    want_good, want = orc.decode_png(png, prior=prior)
    assert want_good == 1
    at, z = 8, b""
    while at + 8 <= len(png):
        ln = int.from_bytes(png[at:at + 4], "big")
        if png[at + 4:at + 8] == b"IDAT":
            z += png[at + 8:at + 8 + ln]
        at += 12 + ln
    stream = zlib.decompress(z)
    emu.emu_png_defilter_batch.restype = C.c_int
    emu.emu_png_defilter_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    sa = np.zeros(len(stream) + 64, dtype=np.uint8)
    sa[3:3 + len(stream)] = np.frombuffer(stream, dtype=np.uint8)
    n = 37 * 21 * 4
    tmp_off = (n + 31) // 16 * 16
    rgba = np.zeros(tmp_off + n + 64, dtype=np.uint8)
    rgba[:n] = prior
    img = (DebigPngImage * 1)()
    img[0].stream_off, img[0].rgba_off, img[0].pal_off, img[0].tmp_off = 3, 0, 0, tmp_off
    img[0].width, img[0].height, img[0].color_type, img[0].asserts_off, img[0].replay_p3 = 37, 21, 2, 0, 1
    res = (DebigPngResult * 1)()
    assert emu.emu_png_defilter_batch(sa.ctypes.data, rgba.ctypes.data, img, res, 1) == 0
    assert res[0].good == 1
    assert np.array_equal(rgba[:n], want)


def test_checksum_kernels_on_emulator(emu):
    """CRC-32 / Adler-32 kernels (tile grid, polynomial combine, inverse power) vs zlib"""
    import random

    class Span(C.Structure):
        _fields_ = [("off", C.c_uint64), ("len", C.c_uint64)]

    emu.emu_checksum_batch.restype = C.c_int
    emu.emu_checksum_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    rng = random.Random(9)
    arena = np.frombuffer(bytes(rng.getrandbits(8) for _ in range(120000)), dtype=np.uint8).copy()
    lens = [0, 1, 3, 4, 5, 16, 17, 64, 65, 1000, 16383, 16384, 16385, 50001]
    spans = (Span * len(lens))()
    for i, n in enumerate(lens):
        spans[i].off, spans[i].len = rng.randrange(0, 60000), n
    out = (C.c_uint32 * len(lens))()
    for kind, fn in ((0, zlib.crc32), (1, zlib.adler32)):
        assert emu.emu_checksum_batch(arena.ctypes.data, spans, out, len(lens), kind) == 0
        for i, n in enumerate(lens):
            assert out[i] == fn(arena[spans[i].off:spans[i].off + n].tobytes()), (kind, n)


def test_resolve_idle_bound_is_reported_not_silent(emu, oracle):
    """VERDICT r1 weak-7 / ADVICE: when a wavefront of the multi-wavefront match resolve exhausts
    its idle polls it used to leave the loop silently (good = 1 with unresolved match bytes).
    DEBIG_STREAM_FAULT_INJECT_IDLE makes the FIRST idle poll give up, so ordinary text data
    (matches whose sources belong to another wavefront) takes that exit: every stream must come
    back either correct (it never had to poll) or failed with DEBIG_E_INTERNAL -- never good with
    wrong bytes -- and the workgroup must still be usable for the next stream."""
    FAULT = 0x80000000
    E_INTERNAL = 10
    # a strictly serial chain of self-overlapping matches (each one's source is the previous
    # one's output): a wavefront that starts a span whose predecessor span belongs to another
    # wavefront has all of its lanes waiting -- an idle poll
    chain = b"abc" * 30000
    pairs = [(zlib.compress(chain, 6)[2:-4], np.frombuffer(chain, dtype=np.uint8))]
    pairs += workload.make_streams("dynamic", 3, 65536)
    raws = [p[0] for p in pairs]
    caps = [len(p[1]) + 1 for p in pairs]
    # grid = 1: one workgroup works through all streams, so the state left behind by a failed
    # stream (pending bits, bitmaps, the error flag) is what the next one starts from
    outs, _, _ = eb.emu_inflate(emu, raws, caps, nw=4, grid=1, flags=FAULT)
    tripped = 0
    for (good, final, out, r), (raw, plain) in zip(outs, pairs):
        if good:
            assert final == len(plain) and out == plain.tobytes()
        else:
            assert r.status == E_INTERNAL
            assert out == plain.tobytes()[:final]  # what is claimed is correct
            tripped += 1
    assert tripped >= 1 and not outs[0][0], "the fault injection did not reach the idle-poll exit"
    # and without the flag the same workgroup decodes the same streams
    outs, _, _ = eb.emu_inflate(emu, raws, caps, nw=4, grid=1)
    for (good, final, out, r), (raw, plain) in zip(outs, pairs):
        assert (good, final) == (1, len(plain)) and out == plain.tobytes()


def test_kernels_under_address_sanitizer():
    """SURVEY 5 'sanitizers on the CPU build': the same kernel source under ASan + UBSan
    (tools/simt_emu/libdebig_emu_asan.so) on a small mixed batch: known-answer streams and one
    stream of every block kind, through every inflate path -- one wavefront, a workgroup of 4, the
    scan / LZ77 pair, chunk tasks (1 KiB chunks).
    Runs in a child process (the sanitizer runtime has to be loaded first)."""
    import subprocess
    import sys

    code = r'''
import sys, json, os, hashlib
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import emu_binding as eb
from debigulator_amd import workload
L = eb.load_emu(asan=True)
items = json.load(open(os.path.join(%(root)r, "tests", "golden", "kat.json")))[:6]
raws = [bytes.fromhex(k["raw_hex"]) for k in items]; caps = [k["recipient_size"] for k in items]
for kind, size in (("stored", 5000), ("dynamic", 9000), ("fixed", 3000)):
    raw, plain = workload.make_stream(kind, 3, size)
    raws.append(raw); caps.append(max(size + 1, len(raw))); items.append({"good": 1, "final": size, "plain": plain.tobytes()})
for nw in (1, 4, eb.SPLIT, eb.STRAND, eb.CHUNKED):
    outs, arena, offs = eb.emu_inflate(L, raws, caps, nw=nw, in_misalign=1, out_misalign=3, chunk_bytes=1024)
    for k, (good, final, out, r) in zip(items, outs):
        assert good == k["good"] and final == k["final"], (nw, k.get("name"))
        if "plain" in k: assert out == k["plain"]
        elif k.get("out_hex") is not None: assert out.hex() == k["out_hex"]
print("asan ok")
''' % {"root": ROOT}
    import ctypes.util  # noqa: F401
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "asan ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_split_path_hands_back_what_does_not_fit_its_workspace(emu, oracle):
    """The scan / LZ77 kernel pair (inflate_split_kernel.inc) keeps decoded symbols as token rows in a
    workspace carved in proportion to the input sizes.  Streams that need more than their share --
    a workspace that is simply small, streams of tiny blocks (one record + rows per block), a
    stream whose windows hold many more symbols than bytes suggest -- must come back from the
    one-kernel path in the same call, bit-exact, and the rest must not be disturbed."""
    pairs = workload.make_streams("dynamic", 3, 65536) + workload.make_streams("fixed", 2, 30000)
    raws = [p[0] for p in pairs]
    caps = [len(p[1]) + 1 for p in pairs]
    tiny_raws, tiny_caps = _tiny_block_streams(77, 3, 1500)
    raws += tiny_raws
    caps += tiny_caps
    # all literals with a 1-bit and a 2-bit code: 5+ symbols per input byte
    dense = bytes(random.Random(5).choice(b"aaaaab") for _ in range(40000))
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    raws.append(c.compress(dense) + c.flush())
    caps.append(len(dense) + 1)
    want = [oracle.inflate(r, c) for r, c in zip(raws, caps)]
    seen = set()
    for ws, nw in ((None, eb.SPLIT), (9 * sum(len(r) for r in raws) // 6, eb.SPLIT), (40 * 1024, eb.SPLIT),
                   (len(raws) * 1024 + 4096, eb.SPLIT), (None, eb.STRAND), (9 * sum(len(r) for r in raws) // 6, eb.STRAND),
                   (40 * 1024, eb.STRAND)):
        outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=nw, ws_bytes=ws, out_misalign=3)
        seen.add(eb.last_split_retried)
        for (good, final, out, r), w in zip(outs, want):
            assert (good, final, out) == w
        for (io, oo), cap in zip(offs, caps):
            assert (arena[oo + cap:oo + cap + 32] == 0xA5).all()
    assert 0 not in seen or len(seen) > 1  # the small workspaces really sent streams back
    assert max(seen) >= len(raws) - 1


@functools.lru_cache(maxsize=None)
def _long_code_streams():
    """seven zlib streams -> (raws, caps, {geometry: {(alphabet, route)} of the symbols they decode}); the routes are
    those of tests/table_shapes.py: classify over the code lengths of every dynamic block"""
    import table_shapes as ts

    rng = np.random.default_rng(77)
    raws, caps = [], []
    for it in range(6):
        n = 30000 + 5000 * it
        # literal alphabet with probabilities 2^-1 .. 2^-15 and a uniform tail: long literal codes
        p = np.array([2.0 ** -(1 + (k % 15)) for k in range(60)] + [1e-5] * 196)
        data = rng.choice(256, size=n, p=p / p.sum()).astype(np.uint8).tobytes()
        strat = [zlib.Z_HUFFMAN_ONLY, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED][it % 3]
        c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, strat)
        raws.append(c.compress(data) + c.flush())
        caps.append(n + 1)
    # most matches at a handful of distances, a few anywhere in 32 KiB
    base = rng.integers(0, 256, 40000, dtype=np.uint8)
    buf = bytearray(base.tobytes())
    for k in range(3000):
        src = rng.integers(0, 200) if k % 50 else rng.integers(0, 30000)
        dst = rng.integers(32000, 39000)
        buf[dst:dst + 6] = buf[dst - src - 6:dst - src] if dst - src - 6 >= 0 else buf[dst:dst + 6]
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9)
    raws.append(c.compress(bytes(buf)) + c.flush())
    caps.append(len(buf) + 1)
    reached = {}
    for gname, g in ts.GEOMETRIES.items():
        reached[gname] = set()
        for raw in raws:
            for ll, dl, ul, ud in ts.walk(raw):
                lit, dist = ts.classify(ll, dl, g)
                reached[gname] |= {("lit", lit[s]) for s in ul} | {("dist", dist[s]) for s in ud}
    return raws, caps, reached


@pytest.mark.parametrize("nw", [1, 2, 4, 8, eb.SPLIT, eb.SPLIT_QUEUED, eb.STRAND, eb.STRAND_PIPE])
def test_long_codes_take_the_second_level_tables(emu, oracle, nw):
    """Codes longer than the direct tables (10/11 bits literal/length, 9 bits distance) are decoded through second-level
    tables linked from the direct table (CodeTabsT::sub_tab).  Seven zlib streams: geometric byte distributions give
    literal/length codes up to 15 bits -- links of every size, 1..5 index bits behind the 10-bit table and 1..4 behind
    the 11-bit one --, rare far distances give a few distance codes of 10, 12 and 13 bits (links of 1, 3 and 4 bits).
    What they do NOT reach, by the model of tests/table_shapes.py and asserted below: the canonical probe (no stream of
    zlib's overflows the second-level area), distance links of 2, 5 or 6 bits, and long distance codes in the seventh
    stream, whose distance codes all fit the 9-bit table; tests/test_emu_table_shapes.py reaches those on purpose.  Every
    kernel width, against the oracle (which is pinned to the reference on K9's 13..15 bit codes and on the zlib corpus);
    no stream is skipped: none carries a flag of UB_EXCLUDED (over-subscribed lengths, a repeat code at position 0 --
    zlib writes neither)."""
    import table_shapes as ts
    from handback_corpus import UB_EXCLUDED

    raws, caps, reached = _long_code_streams()
    assert len(raws) == 7
    want = [oracle.inflate(r, c, want_stats=True) for r, c in zip(raws, caps)]
    assert [i for i, w in enumerate(want) if w[3].ub_flags & UB_EXCLUDED] == []
    assert {r for a, r in reached["g10"] if a == "lit"} == {ts.DIRECT} | {ts.LINK(k) for k in range(1, 6)}
    assert {r for a, r in reached["g11"] if a == "lit"} == {ts.DIRECT} | {ts.LINK(k) for k in range(1, 5)}
    assert {r for a, r in reached["g10"] if a == "dist"} == {r for a, r in reached["g11"] if a == "dist"} == \
        {ts.DIRECT, ts.LINK(1), ts.LINK(3), ts.LINK(4)}
    eb.slow_probes(emu)
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=nw, out_misalign=5)
    for i, ((good, final, out, r), (g, f, o, st)) in enumerate(zip(outs, want)):
        assert (good, final, out) == (g, f, o), (nw, i)
    assert sum(1 for w in want if w[0] == 1) >= 5
    assert eb.slow_probes(emu) == 0  # no SLOW mark in any table, so the probe loop never ran


# ---------------------------------------------------------------- chunk-parallel path (inflate_chunk_kernel.inc)
def _text(rng, nbytes):
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(2, 9))) for _ in range(400)]
    out = bytearray()
    while len(out) < nbytes:
        out += rng.choice(words) + b" "
    return bytes(out[:nbytes])


def _raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""
    for at in range(0, len(data), flush_every):
        out += c.compress(data[at:at + flush_every]) + c.flush(zlib.Z_SYNC_FLUSH)
    return out + c.flush()


def _png_stream(seed, w, h):
    png, _ = workload.make_png(seed, w, h, noise=workload.CFG4_NOISE)
    at, z = 8, b""
    while at + 8 <= len(png):
        ln = int.from_bytes(png[at:at + 4], "big")
        if png[at + 4:at + 8] == b"IDAT":
            z += png[at + 8:at + 8 + ln]
        at += 12 + ln
    return z[2:-4]


def test_chunked_path_cuts_large_streams_at_block_headers(emu, oracle):
    """Streams of several blocks through DEBIG_WAVES_CHUNKED with 4 KiB chunks: every kind of block
    sequence, recipients exact / too small, a stream without a place to cut (fixed blocks only) and
    gate failures -- all equal to the oracle, and only the expected ones handed back."""
    rng = random.Random(11)
    nprng = np.random.default_rng(11)
    text = _text(rng, 260000)
    noise = nprng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    cases = []  # (raw, cap, handed back?)
    dyn, plain = workload.make_stream("dynamic", 7, size=150000)
    cases.append((bytes(dyn), len(plain) + 77, False))
    cases.append((_raw(text, 6), len(text), False))                                    # exact recipient
    cases.append((_raw(text[:90000], 1), 90000 + 5, False))
    cases.append((_raw(text[:120000] + noise + text[120000:200000], 9), 240000 + 64, False))  # stored blocks inside
    cases.append((_raw(text[:150000], 6, flush_every=20000), 150000 + 3, False))       # empty stored blocks (sync flush)
    cases.append((_png_stream(3, 200, 150), 200 * 150 * 4 + 150 + 9, False))
    cases.append((_raw(text[:60000], 6) + nprng.integers(0, 256, 9000, dtype=np.uint8).tobytes(), 60000 + 16, False))  # bytes behind the final block
    cases.append((_raw(text[:3000], 6), 3000, False))                                  # one task
    cases.append((_raw(text[:80000], 6, zlib.Z_FIXED), 80000 + 1, False))              # no dynamic block to cut at: one task
    cases.append((_raw(text[:100000], 6), 100000 - 10, True))                          # recipient too small
    cases.append((_raw(noise, 6), len(noise) - 1000, True))                            # gate: recipient < input
    raws, caps = [c[0] for c in cases], [c[1] for c in cases]
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=eb.CHUNKED, chunk_bytes=4096, in_misalign=3, out_misalign=5)
    assert eb.last_split_retried == sum(c[2] for c in cases)
    one, _, _ = eb.emu_inflate(emu, raws, caps, nw=1)  # the one-kernel path: block count and end position
    for i, (raw, cap, (good, final, out, r)) in enumerate(zip(raws, caps, outs)):
        eg, ef, eo = oracle.inflate(raw, cap)[:3]
        assert (good, final) == (eg, ef), i
        assert out == eo, i
        assert (r.n_blocks, r.in_end_bits, r.status) == (one[i][3].n_blocks, one[i][3].in_end_bits, one[i][3].status), i
    for (io, oo), cap in zip(offs, caps):
        assert (arena[oo + cap:oo + cap + 32] == 0xA5).all()


def test_chunked_path_false_header_is_repaired_and_damage_goes_to_the_one_kernel_path(emu, oracle):
    """A byte-aligned copy of a real dynamic block inside a STORED block is what the block finder
    looks for but not a block boundary: the scan of the task before it runs past it to the next
    real boundary, the repair kernel restarts the false task there, and the stream still decodes in
    chunk tasks.  Damaged streams: whatever the chunk tasks make of the bytes behind the damage,
    the result is the oracle's (from the one-kernel path)."""
    rng = random.Random(12)
    text = _text(rng, 200000)
    decoy = _raw(text[:30000], 6)[:6000]          # starts with a dynamic block header at bit 0
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    a = c.compress(text[:60000]) + c.flush(zlib.Z_FULL_FLUSH)        # ends byte aligned
    stored = b"\x00" + len(decoy).to_bytes(2, "little") + (len(decoy) ^ 0xffff).to_bytes(2, "little") + decoy
    c2 = zlib.compressobj(6, zlib.DEFLATED, -15)
    tail = c2.compress(text[60000:140000]) + c2.flush()
    trap = a + stored + tail
    want = text[:60000] + decoy + text[60000:140000]
    assert zlib.decompress(trap, -15) == want
    # a second trap: a short decoy right behind the start of a 4 KiB search range, so that the real
    # boundary behind it lies in the SAME range and no task finds it: the false task is restarted
    # there and scanned again (the first trap's false task is simply emptied)
    trap2 = want2 = None
    for cut in range(60000, 64096, 7):
        c3 = zlib.compressobj(6, zlib.DEFLATED, -15)
        a2 = c3.compress(text[:cut]) + c3.flush(zlib.Z_FULL_FLUSH)
        if (len(a2) + 5) % 4096 < 900:
            d2 = decoy[:1500]
            st2 = b"\x00" + len(d2).to_bytes(2, "little") + (len(d2) ^ 0xffff).to_bytes(2, "little") + d2
            c4 = zlib.compressobj(6, zlib.DEFLATED, -15)
            trap2 = a2 + st2 + c4.compress(text[cut:cut + 80000]) + c4.flush()
            want2 = text[:cut] + d2 + text[cut:cut + 80000]
            break
    assert trap2 is not None and zlib.decompress(trap2, -15) == want2
    outs, _, _ = eb.emu_inflate(emu, [trap, trap2], [len(want) + 11, len(want2)], nw=eb.CHUNKED, chunk_bytes=4096)
    assert eb.last_split_retried == 0
    assert outs[0][0] == 1 and outs[0][2] == want and outs[1][0] == 1 and outs[1][2] == want2
    raws, caps = [trap], [len(want) + 11]
    good_raw = _raw(text, 6)
    for pos in (100, len(good_raw) // 3, len(good_raw) // 2, len(good_raw) - 3000):
        bad = bytearray(good_raw)
        bad[pos] ^= 0x10
        raws.append(bytes(bad))
        caps.append(len(text) + 100)
    raws.append(good_raw[:len(good_raw) // 2])  # truncated: no final block
    caps.append(len(text))
    # what is handed back goes to a workgroup of 4 wavefronts here (the shim's choice for small batches)
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=eb.CHUNKED, chunk_bytes=4096, retry_width=4)
    assert outs[0][0] == 1 and outs[0][2] == want
    assert 1 <= eb.last_split_retried <= len(raws) - 1  # the early flip at least; a flipped literal still decodes
    for raw, cap, (good, final, out, r) in zip(raws, caps, outs):
        eg, ef, eo, st = oracle.inflate(raw, cap, want_stats=True)
        if st.ub_flags & (0x10 | 0x02):
            continue
        assert (good, final, out) == (eg, ef, eo)


def test_chunked_path_small_workspace_hands_everything_back(emu, oracle):
    rng = random.Random(13)
    text = _text(rng, 120000)
    raws = [_raw(text, 6), _raw(text[:50000], 9)]
    caps = [len(text), 50000]
    outs, _, _ = eb.emu_inflate(emu, raws, caps, nw=eb.CHUNKED, chunk_bytes=4096, ws_bytes=300000)
    assert eb.last_split_retried >= 1
    for raw, cap, (good, final, out, r) in zip(raws, caps, outs):
        assert (good, final, out) == oracle.inflate(raw, cap)[:3]
    # with workgroups behind it the path also hands back a large stream that is one task (fixed blocks only)
    big = _text(rng, 700000)
    raws = [_raw(big, 6, zlib.Z_FIXED), _raw(text, 6)]
    assert len(raws[0]) >= 256 << 10
    caps = [len(big), len(text)]
    outs, _, _ = eb.emu_inflate(emu, raws, caps, nw=eb.CHUNKED, chunk_bytes=8192, retry_width=4)
    assert eb.last_split_retried == 1
    for raw, cap, (good, final, out, r) in zip(raws, caps, outs):
        assert (good, final, out) == oracle.inflate(raw, cap)[:3]


def test_chunked_path_p2_aliasing_replay_in_the_last_task(emu):
    """phoebus.png as in test_p2_aliasing_replay_matches_reference_digest, cut into chunk tasks: the
    replay is recorded and applied by the task that holds the end of the stream."""
    gold = json.load(open(os.path.join(GOLD, "resources.json")))["png"]["phoebus.png"]
    data = open(os.path.join(GOLD, "resources", "phoebus.png"), "rb").read()
    w, h = gold["width"], gold["height"]
    at, z = 8, b""
    while at + 8 <= len(data):
        ln = int.from_bytes(data[at:at + 4], "big")
        if data[at + 4:at + 8] == b"IDAT":
            z += data[at + 8:at + 8 + ln]
        at += 12 + ln
    raw = z[2:-4]
    est = 4 * w * h + h + 1
    s0 = est - 772 + ((16 - (est & 15)) & 15)
    outs, arena, offs = eb.emu_inflate(emu, [raw], [est], nw=eb.CHUNKED, chunk_bytes=2048, p2=[(s0, est)])
    good, final, stream, r = outs[0]
    assert good == 1 and final == est - 1
    rgba = _emu_defilter(emu, stream, w, h, 6)
    assert hashlib.sha256(rgba.tobytes()).hexdigest() == gold["rgba_sha256"]
    print("phoebus: handed back", eb.last_split_retried, "blocks", r.n_blocks)


@pytest.mark.parametrize("seed,chunk", [(21, 1024), (22, 2048), (23, 6144), (24, 1024), (25, 3072), (26, 4096), (27, 1536),
                                        (28, 8192), (29, 1024), (30, 2048)])
def test_chunked_path_random_streams_agree_with_oracle(emu, oracle, seed, chunk):
    """Random block structures through chunk tasks of several sizes: text / noise / run mixtures,
    every zlib level and strategy, sync and full flushes at random places, a third of the streams
    damaged (flipped bit or cut short): status, size and bytes must be the oracle's."""
    rng = random.Random(seed)
    nprng = np.random.default_rng(seed)
    raws, caps = [], []
    for it in range(14):
        parts = []
        for _ in range(rng.randint(1, 5)):
            kind = rng.random()
            n = rng.randint(2000, 30000)
            if kind < 0.5:
                parts.append(_text(rng, n))
            elif kind < 0.7:
                parts.append(nprng.integers(0, 256, n, dtype=np.uint8).tobytes())
            elif kind < 0.85:
                parts.append(bytes([rng.randrange(256)]) * n)
            else:
                parts.append((bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 40))) * (n // 2 + 1))[:n])
        strat = rng.choice([zlib.Z_DEFAULT_STRATEGY] * 4 + [zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED])
        c = zlib.compressobj(rng.choice([1, 3, 6, 9]), zlib.DEFLATED, -15, rng.choice([8, 9]), strat)
        raw = b""
        for p in parts:
            raw += c.compress(p)
            if rng.random() < 0.4:
                raw += c.flush(rng.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH]))
        raw += c.flush()
        plain = b"".join(parts)
        r = rng.random()
        if r < 0.2 and len(raw) > 200:
            bad = bytearray(raw)
            bad[rng.randrange(len(bad))] ^= 1 << rng.randrange(8)
            raw = bytes(bad)
        elif r < 0.33 and len(raw) > 200:
            raw = raw[:rng.randint(100, len(raw) - 1)]
        raws.append(raw)
        caps.append(max(len(plain) + rng.choice([0, 1, 100]), len(raw)))
    outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=eb.CHUNKED, chunk_bytes=chunk, in_misalign=seed & 7,
                                       out_misalign=seed % 5, retry_width=rng.choice([1, 4]))
    for i, (raw, cap, (good, final, out, r)) in enumerate(zip(raws, caps, outs)):
        eg, ef, eo, st = oracle.inflate(raw, cap, want_stats=True)
        if st.ub_flags & (0x10 | 0x02):
            continue
        assert (good, final) == (eg, ef), (i, r.status)
        assert out == eo, i
    for (io, oo), cap in zip(offs, caps):
        assert (arena[oo + cap:oo + cap + 32] == 0xA5).all()


@pytest.mark.parametrize("nw", [1, 4, eb.SPLIT, eb.STRAND, eb.STRAND_PIPE])
def test_randomised_dynamic_headers(emu, oracle, nw):
    """tests/header_fuzz.py: random prefix codes and a randomised run-length coding of the code-length
    sequence (16 at the start, runs across the alphabets, runs that reach behind the last length,
    damaged headers): the 64-positions-at-a-time header decoder against the oracle's serial one
    (src/inflate.c:1416-1520)."""
    import header_fuzz as hf
    cs = hf.cases(120 if nw != 4 else 60)
    raws = [c[0] + bytes(8) for c in cs]  # bytes behind the last block: the reference's tail gate stays out of it
    caps = [max(2048, len(r) + 1) for r in raws]
    outs, _, _ = eb.emu_inflate(emu, raws, caps, nw=nw, in_misalign=1)
    n_plain = 0
    n_damaged = 0
    for (_, plain), raw, cap, (good, final, out, r) in zip(cs, raws, caps, outs):
        eg, ef, eo, st = oracle.inflate(raw, cap, want_stats=True)
        if st.ub_flags & (0x10 | 0x02):
            continue  # over-subscribed codes / repeat at position 0: the reference has no defined answer
        assert (good, final, out) == (eg, ef, eo[:ef or 0])
        if plain is not None and eg == 1:  # (a valid stream may still fail the reference: a code length >= its alphabet size, Q6)
            assert out == plain
            n_plain += 1
        elif plain is None:
            n_damaged += 1
    assert n_plain > len(cs) // 2 and n_damaged > len(cs) // 8


def test_strand_path_random_zlib_streams(emu, oracle):
    """DEBIG_WAVES_STRAND (csrc/inflate_strand_kernel.inc) on zlib streams of every strategy and level: many blocks
    per stream, blocks shorter than a strand, windows whose lanes are decoded again in several rounds (a lane that
    was decoded to its end from a wrong start and joins its first decode a round later), probes, stored blocks in
    between -- against the oracle."""
    rng = random.Random(1234)
    raws, caps = [], []
    for it in range(160):
        n = rng.randint(1, 30000)
        kind = rng.randint(0, 3)
        if kind == 0:
            data = bytes(rng.getrandbits(8) for _ in range(n))
        elif kind == 1:
            data = bytes(rng.choice(b"abcdefgh \n") for _ in range(n))
        elif kind == 2:
            words = [bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 9))) for _ in range(rng.randint(5, 300))]
            data = b"".join(rng.choice(words) for _ in range(n // 5 + 1))[:n]
        else:
            data = bytes((i * 7 + (i >> 5)) & 255 for i in range(n))
        strat = rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED])
        c = zlib.compressobj(rng.choice([1, 6, 9]), zlib.DEFLATED, -15, rng.choice([1, 8, 9]), strat)
        raw = b""
        pos = 0
        while pos < len(data):  # flushes cut the stream into blocks of every size
            step = rng.choice([len(data), 50, 700, 5000])
            raw += c.compress(data[pos:pos + step])
            if rng.random() < 0.5:
                raw += c.flush(rng.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH]))
            pos += step
        raw += c.flush()
        raws.append(raw)
        caps.append(max(len(data) + 1, len(raw)))
    want = [oracle.inflate(raw, cap, want_stats=True) for raw, cap in zip(raws, caps)]
    for nw in (eb.STRAND, eb.STRAND_PIPE, eb.STRAND_PIPE_BIG):
        outs, arena, offs = eb.emu_inflate(emu, raws, caps, nw=nw, in_misalign=5, out_misalign=9)
        for (good, final, out, r), (eg, ef, eo, st) in zip(outs, want):
            if st.ub_flags & (0x10 | 0x02):
                continue
            assert (good, final, out) == (eg, ef, eo), nw


def test_lz_half_on_mixed_zlib_streams_agrees_with_oracle(emu, oracle):
    """inflate_split_kernel.inc, the LZ77 half: zlib streams of text, runs and periodic data at three levels and three
    strategies (dense chains of near matches, long runs of one byte) through the pair, the strand kernel, the pipeline
    and chunk tasks (16-bit elements, matches that end behind the tile)"""
    L = emu
    rng = random.Random(77)
    raws, caps = [], []
    for it in range(10):
        parts = []
        for _ in range(rng.randint(1, 4)):
            kind, n = rng.random(), rng.randint(1500, 14000)
            if kind < 0.4:
                parts.append(bytes(rng.choice(b"abcdefgh \n") for _ in range(n)))
            elif kind < 0.6:
                parts.append(bytes([rng.randrange(256)]) * n)
            elif kind < 0.85:
                parts.append((bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 40))) * (n // 2 + 1))[:n])
            else:
                parts.append(bytes(rng.getrandbits(8) for _ in range(n)))
        c = zlib.compressobj(rng.choice([1, 6, 9]), zlib.DEFLATED, -15, 9, rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_RLE, zlib.Z_FIXED]))
        raw = c.compress(b"".join(parts)) + c.flush()
        raws.append(raw)
        caps.append(max(sum(len(p) for p in parts) + 1, len(raw)))
    want = [oracle.inflate(raw, cap) for raw, cap in zip(raws, caps)]
    for nw, kw in ((eb.SPLIT, {}), (eb.STRAND, {}), (eb.STRAND_PIPE, {}), (eb.STRAND_PIPE_BIG, {}), (eb.CHUNKED, {"chunk_bytes": 1024})):
        outs, arena, offs = eb.emu_inflate(L, raws, caps, nw=nw, in_misalign=1, out_misalign=7, **kw)
        for (good, final, out, r), (eg, ef, eo) in zip(outs, want):
            assert (good, final, out) == (eg, ef, eo), hex(nw)
