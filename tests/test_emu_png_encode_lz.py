"""Level 3 of the PNG encode (csrc/png_encode_lz_kernel.inc) on the CPU lock-step emulator against tests/png_encode_lz_ref.py:
  * run_lz() lays streams, slots, token rows and counts out as tests/test_emu_png_encode_dyn.py: run_dynamic() does -- odd stream
    addresses, 16 bytes that nobody owns between two slots and between two token rows, sentinels around every buffer -- and launches
    debig_png_encode_lz_kernel through tests/stage_launch.py.
  * check_lz(), for every task: png_encode_ref.check_task() (zlib inflates the task's bytes ALONE with the 32 KiB in front of the
    chunk as its dictionary), IDENTICAL BYTES and token rows from four launches (grid 0, grid 1 in reversed task order, grid 3,
    grid 0 again), THE EXACT CHECK: the first ntok words of the task's token row are the restated rule's tokens word for word, and
    the task's bytes are, byte for byte, what the restated choice names: the restated dynamic_block(), fixed_block() or the chunk
    stored.
The case named test_tasks_that_break_a_bound_lz hands the kernel wrong tasks on purpose: tests/test_gpu_png_encode_lz.py leaves it out."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_dyn_ref as D  # noqa: E402
import png_encode_lz_ref as Z  # noqa: E402
import png_encode_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
import test_emu_png_encode as E  # noqa: E402
import test_emu_png_encode_dyn as Y  # noqa: E402
from emu_binding import load_emu  # noqa: E402

FILL, GAP, CHUNK, PATTERN32 = E.FILL, E.GAP, R.CHUNK, E.PATTERN32
LZ = "png_encode_lz"
KERNELS = dict(Y.KERNELS, **{LZ: (SL.IN, SL.OUT, SL.OUT, SL.TASKS, SL.OUT)})


class ZTask(C.Structure):  # include/debig_hip.h: debig_png_encode_lz_task
    _fields_ = E.DTask._fields_ + [("token_off", C.c_uint64), ("token_cap", C.c_uint32), ("row_stride", C.c_uint32)]


assert C.sizeof(ZTask) == 80
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
    """tests/stage_launch.py learns the launchers for the length of one test (its table is another test's yardstick)"""
    for name, roles in KERNELS.items():
        monkeypatch.setitem(SL.KERNELS, name, roles)


def run_lz(streams, bpp=1, stride=0, grid=0, reverse=False, flags=0, keep=None, spoil=None, caps=None):
    """streams: bytes each; keep(stream index, chunk index) -> False leaves a task out; caps(chunk_len) -> slot_cap
    -> [[the task's slot (a copy) per chunk] per stream], [[count per chunk] per stream], [[token row (uint32, a copy) per chunk] per stream], tasks"""
    soff, at, sl, tk, tasks, idx = [], 0, GAP, GAP, [], 0
    for s in streams:
        at += 1 + -at % 2  # odd addresses
        soff.append(at)
        at += len(s)
    arena = E._aligned(at + 16, 0x5A)
    for s, o in zip(streams, soff):
        arena[o: o + len(s)] = np.frombuffer(s, np.uint8)
    before = arena.copy()
    where = []
    for i, s in enumerate(streams):
        cuts = R.chunks(len(s))
        where.append([])
        for k, (off, ln) in enumerate(cuts):
            cap = R.slot_bytes(ln) if caps is None else caps(ln)
            where[i].append((sl, cap, idx, tk, 4 * ln))
            if keep is None or keep(i, k):
                tasks.append(ZTask(stream_off=soff[i], stream_len=len(s), chunk_off=off, slot_off=sl, chunk_len=ln, slot_cap=cap, level=3, bpp=bpp,
                                   last=int(k == len(cuts) - 1), count_idx=idx, flags=flags, token_off=tk, token_cap=4 * ln, row_stride=stride))
            sl += cap + 16  # 16 bytes that nobody owns between two slots ...
            tk += 4 * ln + 16  # ... and between two token rows
            idx += 1
    idx += 3  # (words that no task has)
    obuf = E._aligned(sl + GAP, FILL)
    tbuf = E._aligned(tk + GAP, FILL)
    cfull = E._aligned(2 * GAP + 4 + 4 * idx, FILL)
    cbuf = cfull[GAP + 4:]
    if spoil:
        spoil(tasks)
    if reverse:
        tasks = tasks[::-1]
    assert SL.launch(LZ, arena, obuf, tbuf, (ZTask * max(len(tasks), 1))(*tasks), cbuf, len(tasks), grid, emu=_emu) == 0
    assert arena.tobytes() == before.tobytes(), "the streams were written"
    assert (obuf[:GAP] == FILL).all() and (obuf[sl:] == FILL).all(), "a sentinel around the slots was written"
    assert (tbuf[:GAP] == FILL).all() and (tbuf[tk:] == FILL).all(), "a sentinel around the token rows was written"
    assert (cfull[:GAP + 4] == FILL).all() and (cbuf[4 * idx:] == FILL).all(), "a sentinel around the counts was written"
    counts = cbuf[: 4 * idx].view(np.uint32)
    assert (counts[idx - 3:] == PATTERN32).all()
    out, cnt, rows = [], [], []
    for i, w in enumerate(where):
        for k, (o, cap, _, t, tcap) in enumerate(w):
            assert (obuf[o + cap: o + cap + 16] == FILL).all(), "the bytes behind a slot were written"
            assert (tbuf[t + tcap: t + tcap + 16] == FILL).all(), "the bytes behind a token row were written"
            if keep is not None and not keep(i, k):
                assert (tbuf[t: t + tcap] == FILL).all(), "the token row of a task that is not in the launch was written"
        out.append([obuf[o: o + cap].copy() for o, cap, _, _, _ in w])
        cnt.append([int(counts[j]) for _, _, j, _, _ in w])
        rows.append([tbuf[t: t + tcap].copy().view(np.uint32) for _, _, _, t, tcap in w])
    return out, cnt, rows, tasks


def check_lz(streams, bpp=1, stride=0, flags=0, keep=None, caps=None):
    """-> [[(the task's bytes, what the restated choice says, the restated tokens) per chunk] per stream], after every check the
    module's docstring lists"""
    runs = [run_lz(streams, bpp, stride, grid=g, reverse=r, flags=flags, keep=keep, caps=caps) for g, r in ((0, False), (1, True), (3, False), (0, False))]
    out, cnt, rows, _ = runs[0]
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
            L, dist = Z.lengths(s, off, ln, bpp, stride)
            tokens, deferred = Z.walk(s, off, ln, L, dist)
            words = np.array(Z.token_words(tokens), np.uint32)
            for other_out, other_cnt, other_rows, _ in runs:
                assert other_cnt[i][k] == n and other_out[i][k][:n].tobytes() == data, (i, k, "the bytes depend on the grid, the order or the run")
                got = other_rows[i][k][: len(words)]
                assert np.array_equal(got, words), (i, k, "THE EXACT CHECK", np.nonzero(got != words)[0][:4], len(words))
            R.check_task(data, k, s)
            assert D.expand(tokens, s[:off]) == s[off: off + ln]
            what = D.choice(tokens, ln, last, flags, None if caps is None else caps(ln))
            want = D.dynamic_block(tokens, last) if what == "dynamic" else Z.fixed_block(tokens, last) if what == "fixed" else Z.stored_block(s[off: off + ln], last)
            assert data == want, (i, k, what, len(data), len(want))
            blks = D.blocks(data)
            assert blks[0]["btype"] == {"dynamic": 2, "fixed": 1, "stored": 0}[what]
            assert [b["final"] for b in blks] == [0] * (len(blks) - 1) + [int(last)]
            if not flags:
                assert n <= 5 + ln + (0 if last else 5), "longer than stored"
            res[i].append((data, what, tokens))
    return res


def _whats(res):
    return [w for r in res for _, w, _ in r]


def _matches(res):
    return [t for r in res for x in r if x for t in x[2] if isinstance(t, tuple)]


_text = Y._text


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_chunk_lengths(n):
    res = check_lz([_text(n)], bpp=3, stride=3 * 40 + 1)
    assert E.zlib_inflate(b"".join(d for d, _, _ in res[0])) == _text(n)
    if n >= 63:
        assert _whats(res)[0] == "dynamic"


@pytest.mark.parametrize("n", [258, 259, 321, 322, 323, 384, 385, 600])
def test_runs_of_one_byte_inside_noise(n):
    """the bitmap's word and look-ahead edges: a run that starts at lane 0, at lane 63 and at lane 1 of a step"""
    rng = np.random.default_rng(n)
    for start in (128, 127, 193, 64 * 5 + 63):
        s = bytearray(rng.integers(0, 256, start + n + 300, dtype=np.uint8).tobytes())
        s[start: start + n] = bytes([s[start]]) * n
        s[start + n] = s[start] ^ 1
        s[start - 1] = s[start] ^ 2
        res = check_lz([bytes(s)])
        m = [t for t in _matches(res) if t[1] == 1]
        assert m and m[0][0] == min(n - 1, 258) and sum(ln for ln, _ in m) >= n - 1 - 2, (n, start, m)


def test_a_run_across_a_chunk_seam():
    rng = np.random.default_rng(1)
    noise = rng.integers(0, 64, CHUNK - 100, dtype=np.uint8).tobytes()
    res = check_lz([noise + bytes([9]) * 400 + noise[:50]])
    assert [t for t in res[0][1][2] if isinstance(t, tuple)][0] == (258, 1)  # the second chunk starts inside the run


def _rows_like_the_row_above(S, rows, seed, change=0.02, values=9):
    """rows of S bytes, each the row above with a few bytes changed; the first row is runs of random length"""
    rng = np.random.default_rng(seed)
    row = np.repeat(rng.integers(0, values, S // 5 + 1), 5)[:S].astype(np.uint8)
    out = []
    for _ in range(rows):
        out.append(row.copy())
        hit = rng.random(S) < change
        row = np.where(hit, rng.integers(0, values, S), row).astype(np.uint8)
    return np.concatenate(out).tobytes()


@pytest.mark.parametrize("case", ["previous_chunk", "first_row", "S_minus_bpp_is_1", "S_is_32768_minus_bpp", "no_stride"])
def test_rows_equal_to_the_row_above(case):
    if case == "previous_chunk":  # rows of 1000: the row above the second chunk's first rows lies in the first chunk
        s, bpp, S = _rows_like_the_row_above(1000, 40, 1), 1, 1000
    elif case == "first_row":  # gp < S on the whole first row: the candidate is not there
        s, bpp, S = _rows_like_the_row_above(700, 3, 2), 3, 700
    elif case == "S_minus_bpp_is_1":
        s, bpp, S = _rows_like_the_row_above(4, 300, 3, change=0.1), 3, 4
    elif case == "S_is_32768_minus_bpp":
        s, bpp, S = _rows_like_the_row_above(32768 - 4, 2, 4, change=0.001), 4, 32768 - 4
    else:
        s, bpp, S = _rows_like_the_row_above(1000, 10, 5), 1, 0
    res = check_lz([s], bpp=bpp, stride=S)
    dists = {d for _, d in _matches(res)}
    if case == "no_stride":
        with_s = check_lz([s], bpp=bpp, stride=1000)
        assert 1000 in {d for _, d in _matches(with_s)}
        assert sum(len(d) for d, _, _ in with_s[0]) < sum(len(d) for d, _, _ in res[0])
    elif case == "S_minus_bpp_is_1":
        assert Z.fixed_distances(bpp, S) == [1, 3, 4, 7]
    else:
        assert S in dists, sorted(dists)[:8]
    if case == "previous_chunk":
        first = [t for t in res[0][1][2] if isinstance(t, tuple)][0]
        assert first[1] == 1000  # 32768 is no multiple of 1000: the chunk starts inside a row and copies the row above


@pytest.mark.parametrize("shift", [-1, 1])
@pytest.mark.parametrize("bpp", [1, 2])
def test_borders_shifted_by_one_pixel_between_rows(shift, bpp):
    """a class border that moves one pixel per row: the row above matches at S + bpp (the border moves right) or S - bpp (left), and
    at S itself away from the border"""
    rng = np.random.default_rng(7 + bpp)
    W, H = 300, 60
    base = np.repeat(rng.integers(0, 250, (W + 2 * H) // 3 + 2), 3)
    rows = []
    for y in range(H):  # pixel x of row y is pixel x - shift of the row above
        px = base[H + np.arange(W) - y * shift]
        rows.append(np.concatenate([[0], np.repeat(px, bpp)]).astype(np.uint8))
    s = np.concatenate(rows).tobytes()
    S = 1 + W * bpp
    res = check_lz([s], bpp=bpp, stride=S)
    dists = {d for _, d in _matches(res)}
    assert (S + bpp if shift == 1 else S - bpp) in dists, sorted(dists)
    # ... and a still image of the same rows matches at S
    still = np.concatenate([rows[0]] * 8).tobytes()
    assert S in {d for _, d in _matches(check_lz([still], bpp=bpp, stride=S))}


PLANT = (130, 100, 70)  # the distances of the planted sources: the later position's is the nearer one, so the table holds it


def _plant(s, q, lens):
    """L(q + j) = lens[j] (ascending): position q + j agrees with the bytes PLANT[j] in front of it for exactly lens[j] bytes.  Bytes
    from 128 up occur nowhere else in the stream: they end a match."""
    j = len(lens) - 1
    src = q + j - PLANT[j]
    s[q + j: q + j + lens[j]] = s[src: src + lens[j]]
    s[q + j + lens[j]] = 128 + j
    for j in range(len(lens) - 2, -1, -1):  # the sources of the positions in front take the bytes that now stand there
        src = q + j - PLANT[j]
        s[src: src + lens[j]] = s[q + j: q + j + lens[j]]
        s[src + lens[j]] = 140 + j


DEFERRALS = {"at62": 64 * 48 + 62, "at63": 64 * 51 + 63, "twice": 3400, "l15": 3600, "l16": 3800}


def deferral_stream():
    """noise of 7 bits with planted copies, so that L(q) and L(q + 1) are what each case of the issue says"""
    rng = np.random.default_rng(2026)
    s = bytearray(rng.integers(0, 128, 6000, dtype=np.uint8).tobytes())
    _plant(s, DEFERRALS["at62"], (5, 9))  # a deferral at q % 64 == 62
    _plant(s, DEFERRALS["at63"], (5, 9))  # q % 64 == 63: the neighbour is longer and the match is still taken
    _plant(s, DEFERRALS["twice"], (4, 6, 9))  # twice in a row
    _plant(s, DEFERRALS["l15"], (15, 17))  # L(q) = 15 defers
    _plant(s, DEFERRALS["l16"], (16, 17))  # L(q) = 16 does not
    return bytes(s)


def test_deferrals_are_counted_by_the_restatement():
    s, at = deferral_stream(), DEFERRALS
    res = check_lz([s])
    L, dist = Z.lengths(s, 0, len(s), 1, 0)
    tokens, deferred = Z.walk(s, 0, len(s), L, dist)
    starts = list(np.cumsum([0] + [t[0] if isinstance(t, tuple) else 1 for t in tokens]))
    q = at["at62"]
    assert q % 64 == 62 and (L[q], L[q + 1]) == (5, 9) and q in deferred and tokens[starts.index(q + 1)] == (9, 100)
    q = at["at63"]
    assert q % 64 == 63 and (L[q], L[q + 1]) == (5, 9) and q not in deferred and tokens[starts.index(q)] == (5, 130)
    q = at["twice"]
    assert (L[q], L[q + 1], L[q + 2]) == (4, 6, 9) and q in deferred and q + 1 in deferred and tokens[starts.index(q + 2)] == (9, 70)
    q = at["l15"]
    assert (L[q], L[q + 1]) == (15, 17) and q in deferred and tokens[starts.index(q + 1)] == (17, 100)
    q = at["l16"]
    assert (L[q], L[q + 1]) == (16, 17) and q not in deferred and tokens[starts.index(q)] == (16, 130)
    assert deferred == [at["at62"], at["twice"], at["twice"] + 1, at["l15"]] and res[0][0][2] == tokens


@pytest.mark.parametrize("period", [32768, 32769])
def test_the_window_edge(period):
    block = np.random.default_rng(period).integers(0, 64, period, dtype=np.uint8).tobytes()
    res = check_lz([block * 2, block[:300] + bytes(period - 300) + block[:300] + b"end"])
    assert all(d <= 32768 for _, d in _matches(res))
    m = [t for t in res[1][1][2] if isinstance(t, tuple)]
    assert m[0] == (258, 32768) if period == 32768 else all(d < 300 for _, d in m)


def test_a_token_of_more_than_32_bits():
    res = check_lz([Y.far_copy_stream()])
    data, what, _ = res[0][1]
    b = D.blocks(data)[0]
    far = [ln for ln, d in b["matches"] if d == 20000]
    assert what == "dynamic" and b["bits"] >= 32 and max(far) >= 100, (b["bits"], far)


@pytest.mark.parametrize("n", [1, 2, 5, 40, 300])
def test_only_dynamic_on_small_chunks(n):
    s = bytes(range(200, 200 + n)) if n < 50 else np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    for stream in (s, _text(CHUNK) + s):  # as a last chunk, and a first chunk in front of it
        res = check_lz([stream], flags=D.ONLY_DYNAMIC)
        assert all(w == "dynamic" and D.blocks(d)[0]["btype"] == 2 for d, w, _ in res[0])


def test_every_flag_and_every_branch_of_the_choice():
    noise = np.random.default_rng(3).integers(0, 256, CHUNK + 700, dtype=np.uint8).tobytes()
    res = check_lz([noise, bytes(2 * CHUNK + 77), bytes([200, 201, 202]), _text(5000)], stride=100)
    w = _whats(res)
    assert "stored" in w and "fixed" in w and "dynamic" in w
    for flags in (R.NO_STORED, D.ONLY_DYNAMIC, D.ONLY_DYNAMIC | R.NO_STORED):
        check_lz([noise[:2000], bytes([200, 201, 202]), _text(700)], flags=flags, stride=50)
    # ONLY_DYNAMIC where the dynamic block does not fit the slot: what the other flag says, and the same in a larger slot
    for n in range(20, 60):
        s = bytes(range(255, 255 - 4 * n, -4))
        if (D.block_bytes(D.sizes(list(s), n, True)[2], True) + 3) // 4 * 4 > R.slot_bytes(n):
            break
    else:
        pytest.fail("no input whose dynamic block is longer than its slot")
    assert _whats(check_lz([s], flags=D.ONLY_DYNAMIC)) == ["stored"]
    assert _whats(check_lz([s], flags=D.ONLY_DYNAMIC | R.NO_STORED)) == ["fixed"]
    assert _whats(check_lz([s], flags=D.ONLY_DYNAMIC, caps=lambda ln: R.slot_bytes(ln) + 64)) == ["dynamic"]


def test_tasks_not_in_the_launch_keep_their_slots_and_rows():
    s = _text(2 * CHUNK + 500, 3)
    check_lz([s, s[:100], s[5:]], bpp=3, stride=301, keep=lambda i, k: (i + k) % 2 == 0)


def test_tasks_that_break_a_bound_lz():
    s = _text(1500, 4)
    edits = [("chunk_len", 0), ("chunk_off", 1500), ("chunk_len", 1501), ("slot_cap", R.slot_bytes(1500) - 16), ("level", 1), ("level", 2), ("level", 4),
             ("last", 2), ("bpp", 0), ("bpp", 9), ("chunk_len", CHUNK + 1), ("slot_off", None), ("token_off", None), ("token_cap", 4 * 1500 - 1),
             ("row_stride", 3), ("row_stride", 2), ("row_stride", 32768 - 2), ("row_stride", 2 ** 32 - 1)]
    streams = [s] * (len(edits) + 2)

    def spoil(tasks):
        for k, (field, v) in enumerate(edits):
            setattr(tasks[k], field, getattr(tasks[k], field) + 2 if v is None else v)
        tasks[len(edits)].row_stride = 32768 - 3  # the largest that holds

    out, cnt, _, _ = run_lz(streams, bpp=3, stride=100, spoil=spoil, keep=lambda i, k: True)
    for k in range(len(edits)):
        assert cnt[k][0] == PATTERN32 and (out[k][0] == FILL).all(), (k, edits[k])
    for k in (len(edits), len(edits) + 1):
        R.check_task(out[k][0][: cnt[k][0]].tobytes(), 0, s)


# ---- whole files from the kernels: what tests/golden/png_encode_lz.json records -------------------------------------------------------

def blocky_map():
    """the issue's first map: 300 x 400, 21 classes in blocks of 8 x 16"""
    rng = np.random.default_rng(1)
    return np.repeat(np.repeat(rng.integers(0, 21, (38, 26)), 8, 0), 16, 1)[:300, :400]


def curved_map():
    """the issue's second map: 256 x 384, 19 classes with curved borders"""
    y, x = np.mgrid[0:256, 0:384]
    return ((np.sin(x / 23) + np.cos(y / 17) + np.sin((x + y) / 31)) * 3).astype(np.int64) % 19


def golden_inputs():
    """the level-2 golden inputs and the two label maps of the issue's table under filter none"""
    pal = np.random.default_rng(20261023).integers(0, 256, (21, 3), dtype=np.uint8)
    return Y.golden_inputs() + [("blocky_21_classes_none", E.Img(blocky_map(), palette=21), 0, pal, None),
                                ("curved_borders_none", E.Img(curved_map(), palette=21), 0, pal, None)]


def kernels_file(im, filt, palette=None, trns=None, level=3):
    """one PNG file from the filter and the lz kernel (level 2: the dynamic kernel) through the launch seam, the container, the zlib
    header and the two checksums from the restatement and zlib"""
    import zlib

    if level == 2:
        return Y.kernels_file(im, filt, palette, trns)
    streams, flags, _, _ = E.run_filter([im], filt)
    assert flags[0] == 0
    stream = streams[0].tobytes()
    out, cnt, _, _ = run_lz([stream], bpp=im.C * im.depth // 8, stride=Z.host_stride(im.W, im.C, im.depth))
    payload = b"".join(o[:c].tobytes() for o, c in zip(out[0], cnt[0]))
    zdata = b"\x78\x9c" + payload + (zlib.adler32(stream) & 0xFFFFFFFF).to_bytes(4, "big")
    return R.container(im.W, im.H, im.C, im.depth, zdata, palette, trns)


def golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_encode_lz.json")


def test_the_recorded_digests_are_those_of_the_emulator_path():
    rec = json.load(open(golden_path()))
    cases = golden_inputs()
    assert sorted(rec) == sorted(c[0] for c in cases) and len(cases) >= 14
    for name, im, filt, pal, trns in cases:
        data = kernels_file(im, filt, pal, trns)
        assert hashlib.sha256(data).hexdigest() == rec[name], name
        st, got, inf, _, _ = R.samples_of(data)
        assert st == 0 and np.array_equal(got, im.s), name


def test_the_two_label_maps_are_smaller_than_at_level_2():
    """the size condition of the GPU test, confirmed on the emulator first"""
    for name, im, filt, pal, trns in golden_inputs()[-2:]:
        three, two = kernels_file(im, filt, pal, trns), kernels_file(im, filt, pal, trns, level=2)
        print(name, "level 3", len(three), "level 2", len(two), "ratio %.3f" % (len(three) / len(two)))
        assert len(three) < len(two), name
