"""The two PNG-encode kernels (csrc/png_encode_kernel.inc) on the CPU lock-step emulator against tests/png_encode_ref.py:
  * run_filter() lays tensors out one behind the other, each at an address that is a multiple of its element but not of 16, cuts
    them into runs of rows and launches the filter kernel through tests/stage_launch.py.  The streams lie between two sentinels of
    4 KiB, every stream one byte behind the one before, all filled with a pattern: a row that no task owns keeps it.  The flags of
    the images are zero before the launch, the words around them a pattern.  check_filter(): every owned row is BYTE FOR BYTE the
    restatement's, the flags are exactly the images with an element out of range.
  * run_deflate() lays streams out the same way, cuts them into chunks, gives every task its own slot of worst-case size and
    launches the deflate kernel.  check_deflate(): png_encode_ref.check_task() for every task (zlib inflates the task's bytes ALONE,
    with the 32768 stream bytes in front of the chunk as its dictionary, to exactly the chunk; eof only in the last), the blocks as
    the bit reader lists them (level 0: stored only; level 1: fixed Huffman or stored; BFINAL in the last block of the last chunk
    only; a chunk that is not the last ends 00 00 FF FF), the byte count exact (no byte behind the last block), level 1 never longer
    than level 0, and IDENTICAL BYTES from four launches: grid 0, grid 1 in reversed task order, grid 3, grid 0 again.
    The bit-padding cases switch the stored fallback off with the task's test-only flag DEBIG_PNG_ENCODE_NO_STORED.
The cases named test_tasks_that_break_a_bound_* hand the kernels wrong tasks on purpose: tests/test_gpu_png_encode.py leaves them out."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
from emu_binding import load_emu  # noqa: E402

FILL, GAP = 0xEE, 4096
DTYPES = {"uint8": (0, np.uint8), "uint16": (1, np.uint16), "int32": (2, np.int32), "int64": (3, np.int64)}  # DEBIG_PNG_L_*
CHUNK = R.CHUNK
FILTER, DEFLATE = "png_encode_filter", "png_encode_deflate"
KERNELS = {FILTER: (SL.IN, SL.OUT, SL.TASKS, SL.OUT), DEFLATE: (SL.IN, SL.OUT, SL.TASKS, SL.OUT)}


class FTask(C.Structure):  # include/debig_hip.h: debig_png_encode_filter_task
    _fields_ = [("image_off", C.c_uint64), ("stream_off", C.c_uint64), ("w", C.c_uint32), ("h", C.c_uint32), ("row0", C.c_uint32),
                ("rows", C.c_uint32), ("channels", C.c_uint32), ("dtype", C.c_uint32), ("depth", C.c_uint32), ("layout", C.c_uint32),
                ("filter", C.c_uint32), ("palette_entries", C.c_uint32), ("flag_idx", C.c_uint32), ("reserved", C.c_uint32)]


class DTask(C.Structure):  # include/debig_hip.h: debig_png_encode_deflate_task
    _fields_ = [("stream_off", C.c_uint64), ("stream_len", C.c_uint64), ("chunk_off", C.c_uint64), ("slot_off", C.c_uint64),
                ("chunk_len", C.c_uint32), ("slot_cap", C.c_uint32), ("level", C.c_uint32), ("bpp", C.c_uint32), ("last", C.c_uint32),
                ("count_idx", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(FTask) == 64 and C.sizeof(DTask) == 64
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        for name, roles in KERNELS.items():
            fn = getattr(L, "emu_%s_batch" % name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p] * len(roles) + [C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


@pytest.fixture(autouse=True)
def the_launchers_are_known(monkeypatch):
    """tests/stage_launch.py learns the two launchers for the length of one test (its table is another test's yardstick)"""
    for name, roles in KERNELS.items():
        monkeypatch.setitem(SL.KERNELS, name, roles)


def _aligned(n, fill):
    """n bytes of `fill` that start at a multiple of 64 (a view: the launch seam keeps the address's residue on the GPU)"""
    root = np.full(n + 64, fill, np.uint8)
    off = -root.ctypes.data % 64
    return root[off: off + n]


def _launch(name, bufs, tasks, grid, cls):
    assert SL.launch(name, *bufs[:2], (cls * max(len(tasks), 1))(*tasks), bufs[2], len(tasks), grid, emu=_emu) == 0


# ---- the filter kernel -------------------------------------------------------------------------------------------------------------


class Img:
    """one image of the batch: samples (H, W, C) as integers (kept in int64), its tensor dtype, depth, layout and palette size"""

    def __init__(self, samples, dtype="uint8", depth=None, layout="hwc", palette=0):
        s = np.asarray(samples, np.int64)
        self.s = s if s.ndim == 3 else s[:, :, None]
        self.dtype, self.layout, self.palette = dtype, layout, palette
        self.depth = depth or (16 if dtype == "uint16" else 8)
        self.H, self.W, self.C = self.s.shape
        self.rb = self.W * self.C * self.depth // 8

    def tensor_bytes(self):
        t = self.s.transpose(2, 0, 1) if self.layout == "chw" else self.s
        return np.ascontiguousarray(t).astype(DTYPES[self.dtype][1]).reshape(-1).view(np.uint8)

    def in_range(self):
        top = self.palette - 1 if self.palette else (1 << self.depth) - 1
        return bool(((self.s >= 0) & (self.s <= top)).all())


def run_filter(images, filt, rows=None, grid=0, reverse=False, skip=(), spoil=None):
    """-> ([the stream's bytes per image, a copy], the flags uint32 per image, [bool (H,): rows owned by a task], tasks)"""
    ioff, soff, at, st = [], [], 0, GAP
    for im in images:
        es = np.dtype(DTYPES[im.dtype][1]).itemsize
        at += -at % 16 + es
        ioff.append(at)
        at += im.H * im.W * im.C * es
        st += 1
        soff.append(st)
        st += im.H * (1 + im.rb)
    arena = _aligned(at + 16, 0x5A)
    for im, o in zip(images, ioff):
        b = im.tensor_bytes()
        arena[o: o + b.size] = b
    before = arena.copy()
    sbuf = _aligned(st + GAP, FILL)
    n = len(images)
    ffull = _aligned(2 * GAP + 4 + 4 * n, FILL)
    fbuf = ffull[GAP + 4:]  # the flags start 4 bytes behind a multiple of 16
    fbuf[: 4 * n] = 0
    tasks, owned = [], [np.zeros(im.H, bool) for im in images]
    for i, im in enumerate(images):
        if i in skip:
            continue
        for y0, r in (R.row_runs(im.H, im.rb) if rows is None else [(y, min(rows, im.H - y)) for y in range(0, im.H, rows)]):
            tasks.append(FTask(image_off=ioff[i], stream_off=soff[i], w=im.W, h=im.H, row0=y0, rows=r, channels=im.C,
                               dtype=DTYPES[im.dtype][0], depth=im.depth, layout=1 if im.layout == "chw" else 0, filter=filt,
                               palette_entries=im.palette, flag_idx=i))
            owned[i][y0: y0 + r] = True
    if spoil:
        spoil(tasks, owned)
    if reverse:
        tasks = tasks[::-1]
    _launch(FILTER, (arena, sbuf, fbuf), tasks, grid, FTask)
    assert arena.tobytes() == before.tobytes(), "the tensors were written"
    assert (sbuf[:GAP] == FILL).all() and (sbuf[st:] == FILL).all(), "a sentinel around the streams was written"
    assert (ffull[:GAP + 4] == FILL).all() and (fbuf[4 * n:] == FILL).all(), "a sentinel around the flags was written"
    s_at = GAP
    for im, o in zip(images, soff):
        assert (sbuf[s_at: o] == FILL).all(), "the byte between two streams was written"
        s_at = o + im.H * (1 + im.rb)
    streams = [sbuf[o: o + im.H * (1 + im.rb)].copy() for im, o in zip(images, soff)]
    return streams, fbuf[: 4 * n].view(np.uint32).copy(), owned, tasks


def check_filter(images, filt, **kw):
    streams, flags, owned, tasks = run_filter(images, filt, **kw)
    for i, im in enumerate(images):
        got = streams[i].reshape(im.H, 1 + im.rb)
        assert (got[~owned[i]] == FILL).all(), (i, "a row that no task owns was written")
        ok = im.in_range()
        assert flags[i] == (0 if ok or not owned[i].any() else 1), (i, flags)
        if ok:
            want = np.frombuffer(R.filtered_stream(im.s, im.depth, filt), np.uint8).reshape(im.H, 1 + im.rb)
            assert got[owned[i]].tobytes() == want[owned[i]].tobytes(), (i, filt, np.argwhere(got != want)[:4])
    return streams, flags


def _rand(seed, H, W, Cn, depth):
    rng = np.random.default_rng(seed)
    # smooth and noisy rows: adaptive picks every type somewhere
    base = np.cumsum(rng.integers(-3, 4, (H, W, Cn)), axis=1) + np.cumsum(rng.integers(-2, 3, (H, 1, Cn)), axis=0) + (1 << (depth - 1))
    noisy = rng.integers(0, 1 << depth, (H, W, Cn))
    pick = rng.integers(0, 3, (H, 1, 1)) == 0
    return np.clip(np.where(pick, noisy, base), 0, (1 << depth) - 1)


@pytest.mark.parametrize("filt", range(6))
def test_one_pixel_and_one_row_every_channel_count_and_depth(filt):
    images = []
    for Cn in (1, 2, 3, 4):
        for dt in ("uint8", "uint16"):
            d = 16 if dt == "uint16" else 8
            images += [Img(_rand(Cn, 1, 1, Cn, d), dt), Img(_rand(Cn + 9, 1, 7, Cn, d), dt), Img(_rand(Cn + 20, 2, 3, Cn, d), dt, layout="chw")]
    check_filter(images, filt)


def test_the_first_row_under_every_type():
    im = _rand(3, 1, 9, 3, 8)
    raw = R.raw_rows(im, 8)[0].astype(np.int64)
    left = np.concatenate([np.zeros(3, np.int64), raw[:-3]])
    streams = {f: check_filter([Img(im)], f)[0][0] for f in range(5)}
    assert streams[2][1:].tobytes() == streams[0][1:].tobytes() and streams[4][1:].tobytes() == streams[1][1:].tobytes()  # Up = None, Paeth = Sub
    assert streams[3][1:].tolist() == ((raw - left // 2) & 255).tolist()  # Average = left / 2
    assert [int(streams[f][0]) for f in range(5)] == list(range(5))


@pytest.mark.parametrize("rb", [63, 64, 65, 255, 256, 257])
def test_row_bytes_around_the_wavefront_and_the_workgroup(rb):
    check_filter([Img(_rand(rb, 6, rb, 1, 8)), Img(_rand(rb + 1, 5, rb, 1, 8), "int32")], 5)
    check_filter([Img(_rand(rb, 3, rb, 1, 8))], 4)


@pytest.mark.parametrize("filt", [0, 3, 4, 5])
def test_chw_against_hwc(filt):
    for Cn, dt in ((2, "uint8"), (3, "uint8"), (4, "uint16"), (3, "uint16")):
        s = _rand(Cn, 9, 11, Cn, 16 if dt == "uint16" else 8)
        a = check_filter([Img(s, dt, layout="hwc")], filt)[0][0]
        b = check_filter([Img(s, dt, layout="chw")], filt)[0][0]
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dt", ["int32", "int64"])
@pytest.mark.parametrize("depth", [8, 16])
def test_wide_integers_in_range_and_out_of_range(dt, depth):
    good = _rand(depth, 7, 13, 1, depth)
    images = [Img(good, dt, depth)]
    for pos in (0, 45, 7 * 13 - 1):
        for v in (1 << depth, -1) + ((1 << 32,) if dt == "int64" else ()):
            bad = good.copy()
            bad.reshape(-1)[pos] = v
            images.append(Img(bad, dt, depth))
    images.append(Img(good, dt, depth))
    _, flags = check_filter(images, 5)
    assert flags[0] == 0 and flags[-1] == 0 and flags[1:-1].all()


def test_a_palette_index_equal_to_entries():
    rng = np.random.default_rng(5)
    good = rng.integers(0, 21, (9, 17, 1))
    bad = good.copy()
    bad[4, 5, 0] = 21
    _, flags = check_filter([Img(good, palette=21), Img(bad, palette=21), Img(bad, palette=22), Img(bad, "int64", 8, palette=21)], 0)
    assert flags.tolist() == [0, 1, 0, 1]


@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5])
def test_row_runs_cut_at_every_seam(rows):
    for filt in (4, 5):
        check_filter([Img(_rand(rows, 5, 40, 3, 8)), Img(_rand(rows + 5, 5, 21, 2, 16), "uint16", layout="chw")], filt, rows=rows, grid=2)


@pytest.mark.parametrize("reverse", [False, True])
def test_fewer_workgroups_than_tasks_in_both_orders(reverse):
    images = [Img(_rand(k, 6 + k, 30 + k, 1 + k % 4, 8)) for k in range(5)]
    a = check_filter(images, 5, rows=2, grid=3, reverse=reverse)[0]
    b = check_filter(images, 5, rows=2, grid=1, reverse=not reverse)[0]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_images_without_tasks_keep_the_pattern():
    images = [Img(_rand(k, 5, 9, 3, 8)) for k in range(3)]
    streams, flags = check_filter(images, 5, skip=(1,), grid=1)
    assert (streams[1] == FILL).all()


def test_tasks_that_break_a_bound_filter():
    images = [Img(_rand(k, 6, 10, 1, 8)) for k in range(10)]

    def spoil(tasks, owned):
        edits = [("w", 0), ("h", 16385), ("rows", 0), ("row0", 6), ("rows", 7), ("channels", 5), ("dtype", 4), ("depth", 12), ("filter", 6)]
        for k, (field, v) in enumerate(edits):
            setattr(tasks[k], field, v)
            owned[k][:] = False

    check_filter(images, 5, spoil=spoil)  # image 9 is good: its rows are written, the others keep the pattern

    def spoil2(tasks, owned):
        tasks[0].palette_entries = 257
        tasks[1].channels, tasks[1].palette_entries = 3, 4
        tasks[2].dtype = 2  # int32 tensors have one channel ... and an address that is a multiple of 4
        tasks[2].channels = 3
        tasks[3].image_off += 2  # (an odd address)
        tasks[3].dtype = 1
        tasks[3].depth = 16
        tasks[4].layout = 2
        tasks[5].rows, tasks[5].w, tasks[5].h, tasks[5].row0 = 8, 16384, 16384, 0  # over the budget with more than one row
        for k in range(6):
            owned[k][:] = False

    check_filter(images, 5, spoil=spoil2)


# ---- the deflate kernel ------------------------------------------------------------------------------------------------------------


def run_deflate(streams, level, bpp=1, grid=0, reverse=False, flags=0, keep=None, spoil=None):
    """streams: bytes each; keep(stream index, chunk index) -> False leaves a task out of the launch
    -> [[the task's slot (a copy) per chunk] per stream], [[count per chunk] per stream], tasks"""
    soff, at, slots, sl, tasks, idx = [], 0, [], GAP, [], 0
    for s in streams:
        at += 1 + -at % 2  # odd addresses
        soff.append(at)
        at += len(s)
    arena = _aligned(at + 16, 0x5A)
    for s, o in zip(streams, soff):
        arena[o: o + len(s)] = np.frombuffer(s, np.uint8)
    before = arena.copy()
    where = []
    for i, s in enumerate(streams):
        cuts = R.chunks(len(s))
        where.append([])
        for k, (off, ln) in enumerate(cuts):
            cap = R.slot_bytes(ln)
            where[i].append((sl, cap, idx))
            if keep is None or keep(i, k):
                tasks.append(DTask(stream_off=soff[i], stream_len=len(s), chunk_off=off, slot_off=sl, chunk_len=ln, slot_cap=cap,
                                   level=level, bpp=bpp, last=int(k == len(cuts) - 1), count_idx=idx, flags=flags))
            sl += cap + 16  # 16 bytes that nobody owns between two slots
            idx += 1
    idx += 3  # (words that no task has)
    obuf = _aligned(sl + GAP, FILL)
    cfull = _aligned(2 * GAP + 4 + 4 * idx, FILL)
    cbuf = cfull[GAP + 4:]
    if spoil:
        spoil(tasks)
    if reverse:
        tasks = tasks[::-1]
    _launch(DEFLATE, (arena, obuf, cbuf), tasks, grid, DTask)
    assert arena.tobytes() == before.tobytes(), "the streams were written"
    assert (obuf[:GAP] == FILL).all() and (obuf[sl:] == FILL).all(), "a sentinel around the slots was written"
    assert (cfull[:GAP + 4] == FILL).all() and (cbuf[4 * idx:] == FILL).all(), "a sentinel around the counts was written"
    counts = cbuf[: 4 * idx].view(np.uint32)
    assert (counts[idx - 3:] == np.frombuffer(bytes([FILL]) * 4, np.uint32)[0]).all()
    out, cnt = [], []
    for w in where:
        for o, cap, _ in w:
            assert (obuf[o + cap: o + cap + 16] == FILL).all(), "the bytes behind a slot were written"
        out.append([obuf[o: o + cap].copy() for o, cap, _ in w])
        cnt.append([int(counts[j]) for _, _, j in w])
    return out, cnt, tasks


PATTERN32 = int(np.frombuffer(bytes([FILL]) * 4, np.uint32)[0])


def check_deflate(streams, level, bpp=1, flags=0, keep=None):
    """-> [[the task's bytes per chunk] per stream], after every check the module's docstring lists"""
    runs = [run_deflate(streams, level, bpp, grid=g, reverse=r, flags=flags, keep=keep) for g, r in ((0, False), (1, True), (3, False), (0, False))]
    out, cnt, _ = runs[0]
    res = []
    for i, s in enumerate(streams):
        cuts = R.chunks(len(s))
        res.append([])
        for k, (off, ln) in enumerate(cuts):
            if keep is not None and not keep(i, k):
                assert cnt[i][k] == PATTERN32 and (out[i][k] == FILL).all(), (i, k, "the slot of a task that is not in the launch was written")
                res[i].append(None)
                continue
            last = k == len(cuts) - 1
            n = cnt[i][k]
            assert 0 < n <= len(out[i][k]), (i, k, n)
            data = out[i][k][:n].tobytes()
            for other_out, other_cnt, _ in runs[1:]:
                assert other_cnt[i][k] == n and other_out[i][k][:n].tobytes() == data, (i, k, "the bytes depend on the grid, the order or the run")
            R.check_task(data, k, s)
            blks = R.blocks(data)
            stored = 5 + ln + (0 if last else 5)
            assert sum(b["bytes"] for b in blks) == ln
            assert [b["final"] for b in blks] == [0] * (len(blks) - 1) + [int(last)]
            if not last:
                assert blks[-1]["btype"] == 0 and blks[-1]["bytes"] == 0 and data[-4:] == b"\x00\x00\xff\xff"
            if level == 0:
                assert all(b["btype"] == 0 for b in blks) and n == stored
            elif not flags & R.NO_STORED:
                assert n <= stored
                assert n == stored or blks[0]["btype"] == 1  # stored only as the fallback
            res[i].append(data)
    return res


def _payload(tasks):
    return sum(len(t) for t in tasks)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_stream_lengths(n, level):
    rng = np.random.default_rng(n)
    text = np.repeat(rng.integers(0, 40, n // 3 + 1), 3)[:n].astype(np.uint8).tobytes()  # triples: short matches everywhere
    res = check_deflate([text], level, bpp=3)
    assert zlib_inflate(b"".join(res[0])) == text


def zlib_inflate(raw):
    import zlib

    return zlib.decompress(raw, -15)


@pytest.mark.parametrize("n", range(1, 9))
def test_bit_padding_takes_every_residue(n):
    """n bytes >= 144 as a last chunk, the stored fallback switched off by the task's test-only flag: 3 + 9n + 7 bits"""
    s = bytes(range(200, 200 + n))
    data = check_deflate([s], 1, flags=R.NO_STORED)[0][0]
    blks = R.blocks(data)
    assert len(blks) == 1 and blks[0]["btype"] == 1 and blks[0]["end"] == 3 + 9 * n + 7 and len(data) == (blks[0]["end"] + 7) // 8
    # ... and in a chunk that is not the last: n of its bytes take 8 bits, the others 9, an empty stored block behind it
    first = np.random.default_rng(n).integers(144, 256, CHUNK, dtype=np.uint8)
    first[:: CHUNK // n][:n] = 17 + n
    check_deflate([first.tobytes() + s], 1, flags=R.NO_STORED)


def test_literal_code_edges():
    s = bytes([0, 143, 144, 255, 143, 0, 255, 144, 1, 142, 145, 254])
    data = check_deflate([s], 1, flags=R.NO_STORED)[0][0]
    assert R.blocks(data)[0]["end"] == 3 + 8 * 6 + 9 * 6 + 7 and not R.blocks(data)[0]["matches"]


@pytest.mark.parametrize("n", [257, 258, 259, 260, 261, 262, 600])
def test_runs_of_one_byte(n):
    for v in (0, 200):
        data = check_deflate([bytes([7, v]) + bytes([v]) * (n - 1)], 1)[0][0]
        m = R.blocks(data)[0]["matches"]
        assert m and all(d == 1 and ln <= 258 for ln, d in m) and m[0][0] == min(n - 1, 258)
        assert sum(ln for ln, _ in m) >= n - 1 - 2  # a remainder below 3 becomes literals


@pytest.mark.parametrize("period", [2, 3, 4, 6, 8])
def test_periods_of_the_pixel_distances(period):
    rng = np.random.default_rng(period)
    s = (rng.integers(0, 256, period, dtype=np.uint8).tobytes() * 300)[:1500]
    data = check_deflate([s], 1, bpp=period)[0][0]
    m = R.blocks(data)[0]["matches"]
    assert m and all(d == period for _, d in m) and len(data) < 60
    check_deflate([s], 1, bpp=1)  # the same without the hint: the hash table has to find it


def test_a_run_that_straddles_a_chunk_seam_and_a_chunk_that_is_one_back_reference():
    rng = np.random.default_rng(1)
    noise = rng.integers(0, 256, CHUNK - 100, dtype=np.uint8).tobytes()
    s = noise + bytes([9]) * 400 + noise[:50]
    res = check_deflate([s], 1)
    assert R.blocks(res[0][1])[0]["matches"][0] == (258, 1)  # the second chunk starts inside the run
    # a second chunk that is nothing but 200 bytes of the chunk before it
    block = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    res = check_deflate([noise[: CHUNK - 300] + block + block[100:]], 1)
    b = R.blocks(res[0][1])[0]
    assert b["btype"] == 1 and sum(ln for ln, _ in b["matches"]) >= 150 and all(d == 200 for _, d in b["matches"])


@pytest.mark.parametrize("period,copies", [(32768, 2), (32768, 3), (32769, 2), (32769, 3)])
def test_the_window_edge(period, copies):
    """a random block written again at distance 32768 (legal) and 32769 (no match may cross it: zlib rejects a distance past the window)"""
    block = np.random.default_rng(period).integers(0, 256, period, dtype=np.uint8).tobytes()
    res = check_deflate([block * copies], 1)
    assert all(d <= 32768 for t in res[0] for b in R.blocks(t) for _, d in b["matches"])
    # the same edge by construction: 300 random bytes, zeros (one hash bucket) up to the distance, the 300 bytes again
    res = check_deflate([block[:300] + bytes(period - 300) + block[:300] + b"end"], 1)
    m = R.blocks(res[0][1])[0]["matches"]
    if period == 32768:
        assert m[0] == (258, 32768)  # the second chunk starts with the block: the far end of the window is legal
    else:
        assert all(d < 300 for _, d in m)  # one byte further: the block is out of reach


def test_a_candidate_in_front_of_the_stream():
    """the first three bytes again later, and a stream that starts with a run: nothing in front of byte 0 is ever read"""
    s = b"abcXYZabcabc" + bytes(20)
    check_deflate([s, bytes(50), b"aaa", b"aaaa" * 9], 1)
    check_deflate([s[:7]], 1, bpp=8)


def test_the_stored_fallback_and_the_all_zero_stream():
    noise = np.random.default_rng(2).integers(144, 256, CHUNK + 500, dtype=np.uint8).tobytes()
    zero = bytes(2 * CHUNK + 77)
    l1 = check_deflate([noise, zero], 1)
    l0 = check_deflate([noise, zero], 0)
    assert [len(t) for t in l1[0]] == [len(t) for t in l0[0]] and all(b["btype"] == 0 for t in l1[0] for b in R.blocks(t))
    assert _payload(l1[1]) < _payload(l0[1]) // 100
    assert all(len(a) <= len(b) for a, b in zip(l1[0] + l1[1], l0[0] + l0[1]))


def test_tasks_not_in_the_launch_keep_their_slots():
    s = np.repeat(np.random.default_rng(3).integers(0, 9, CHUNK), 3).astype(np.uint8).tobytes()  # three chunks
    check_deflate([s, s[:100], s[5:]], 1, keep=lambda i, k: (i + k) % 2 == 0)


def test_tasks_that_break_a_bound_deflate():
    s = np.repeat(np.random.default_rng(4).integers(0, 9, 500), 3).astype(np.uint8).tobytes()
    streams = [s] * 11
    edits = [("chunk_len", 0), ("chunk_off", 1500), ("chunk_len", 1501), ("slot_cap", R.slot_bytes(1500) - 16), ("level", 2), ("last", 2), ("bpp", 0),
             ("bpp", 9), ("chunk_len", CHUNK + 1), ("slot_off", None)]

    def spoil(tasks):
        for k, (field, v) in enumerate(edits):
            setattr(tasks[k], field, tasks[k].slot_off + 2 if v is None else v)

    for level in (0, 1):
        out, cnt, _ = run_deflate(streams, level, spoil=spoil)
        for k in range(len(edits)):
            assert cnt[k][0] == PATTERN32 and (out[k][0] == FILL).all(), (k, edits[k])
        R.check_task(out[10][0][: cnt[10][0]].tobytes(), 0, s)


# ---- whole files from the two kernels: what tests/golden/png_encode.json records ---------------------------------------------------

def golden_inputs():
    """[(name, Img, filter, level, palette (entries, 3) uint8 or None, trns uint8 or None)]: a dozen small inputs from a seeded generator"""
    rng = np.random.default_rng(20261021)
    pal = rng.integers(0, 256, (21, 3), dtype=np.uint8)
    blocky = np.repeat(np.repeat(rng.integers(0, 21, (9, 12, 1)), 7, axis=0), 5, axis=1)
    ids = np.repeat(np.repeat(rng.integers(0, 3000, (6, 5, 1)), 9, axis=0), 11, axis=1)
    return [("rgb8_adaptive", Img(_rand(1, 40, 33, 3, 8)), 5, 1, None, None),
            ("rgb8_two_chunks", Img(_rand(2, 100, 120, 3, 8)), 5, 1, None, None),
            ("rgb8_chw_paeth", Img(_rand(3, 31, 17, 3, 8), layout="chw"), 4, 1, None, None),
            ("rgba16_sub", Img(_rand(4, 20, 19, 4, 16), "uint16"), 1, 1, None, None),
            ("grey_alpha8_up", Img(_rand(5, 25, 64, 2, 8)), 2, 1, None, None),
            ("grey16_average_stored", Img(_rand(6, 18, 65, 1, 16), "uint16"), 3, 0, None, None),
            ("noise_rgb8", Img(rng.integers(0, 256, (64, 63, 3))), 5, 1, None, None),
            ("palette_none", Img(blocky, palette=21), 0, 1, pal, None),
            ("palette_trns_adaptive", Img(blocky, "int64", 8, palette=21), 5, 1, pal, rng.integers(0, 256, 7, dtype=np.uint8)),
            ("ids_int32_depth16", Img(ids, "int32", 16), 0, 1, None, None),
            ("ids_int64_depth16_adaptive", Img(ids, "int64", 16, layout="chw"), 5, 1, None, None),
            ("one_pixel", Img(np.array([[[200, 100, 0]]])), 5, 1, None, None),
            ("zeros_level0", Img(np.zeros((70, 500, 1), np.int64)), 0, 0, None, None)]


def kernels_file(im, filt, level, palette=None, trns=None):
    """one PNG file from the two kernels through the launch seam (the emulator, or whatever backend the seam is switched to), the
    container, the zlib header and the two checksums from the restatement and zlib"""
    import zlib

    streams, flags, _, _ = run_filter([im], filt)
    assert flags[0] == 0
    stream = streams[0].tobytes()
    out, cnt, _ = run_deflate([stream], level, bpp=im.C * im.depth // 8)
    payload = b"".join(o[:c].tobytes() for o, c in zip(out[0], cnt[0]))
    zdata = b"\x78\x01" + payload + (zlib.adler32(stream) & 0xFFFFFFFF).to_bytes(4, "big")
    return R.container(im.W, im.H, im.C, im.depth, zdata, palette, trns)


def golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_encode.json")


def test_the_recorded_digests_are_those_of_the_emulator_path():
    import hashlib
    import json

    rec = json.load(open(golden_path()))
    cases = golden_inputs()
    assert sorted(rec) == sorted(c[0] for c in cases) and len(cases) >= 12
    for name, im, filt, level, pal, trns in cases:
        data = kernels_file(im, filt, level, pal, trns)
        assert hashlib.sha256(data).hexdigest() == rec[name], name
        st, got, inf, _, _ = R.samples_of(data)
        assert st == 0 and np.array_equal(got, im.s), name
