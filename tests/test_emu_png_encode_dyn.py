"""Level 2 of the PNG encode (csrc/png_encode_dynamic_kernel.inc) on the CPU lock-step emulator against tests/png_encode_dyn_ref.py:
  * run_dynamic() lays streams, slots and counts out as tests/test_emu_png_encode.py: run_deflate() does, gives every task a token
    row of 4 x chunk_len bytes of its own between two sentinels, 16 bytes that nobody owns between two rows, and launches
    debig_png_encode_dynamic_kernel through tests/stage_launch.py.
  * check_dynamic(), for every task: png_encode_ref.check_task() (zlib inflates the task's bytes ALONE with the 32 KiB in front of
    the chunk as its dictionary), IDENTICAL BYTES from four launches (grid 0, grid 1 in reversed task order, grid 3, grid 0 again),
    the sentinels around streams, slots, counts and token rows, and THE EXACT CHECK: the level-1 kernel's output for the same task
    under DEBIG_PNG_ENCODE_NO_STORED is parsed into level 1's tokens; the restated choice then says which block level 2 writes, the
    restated dynamic_block() gives its bytes where that is the dynamic one, the level-1 kernel under the task's flags gives them
    where it is not; the task's bytes are compared with that byte for byte.
  * run_codes() / check_codes(): debig_png_encode_codes_kernel against the restated rule.
The cases named test_tasks_that_break_a_bound_* hand the kernels wrong tasks on purpose: tests/test_gpu_png_encode_dyn.py leaves them out."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_dyn_ref as D  # noqa: E402
import png_encode_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
import test_emu_png_encode as E  # noqa: E402
from emu_binding import load_emu  # noqa: E402

FILL, GAP, CHUNK, PATTERN32 = E.FILL, E.GAP, R.CHUNK, E.PATTERN32
DYNAMIC, CODES = "png_encode_dynamic", "png_encode_codes"
KERNELS = dict(E.KERNELS, **{DYNAMIC: (SL.IN, SL.OUT, SL.OUT, SL.TASKS, SL.OUT), CODES: (SL.IN, SL.OUT, SL.TASKS)})
MAX_COUNT = 1 << 22  # DEBIG_PNG_ENCODE_CODES_MAX_COUNT


class YTask(C.Structure):  # include/debig_hip.h: debig_png_encode_dynamic_task
    _fields_ = E.DTask._fields_ + [("token_off", C.c_uint64), ("token_cap", C.c_uint32), ("reserved2", C.c_uint32)]


class CTask(C.Structure):  # include/debig_hip.h: debig_png_encode_codes_task
    _fields_ = [("counts_off", C.c_uint64), ("lens_off", C.c_uint64), ("n", C.c_uint32), ("limit", C.c_uint32)]


assert C.sizeof(YTask) == 80 and C.sizeof(CTask) == 24
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


def run_dynamic(streams, bpp=1, grid=0, reverse=False, flags=0, keep=None, spoil=None, caps=None):
    """streams: bytes each; keep(stream index, chunk index) -> False leaves a task out; caps(chunk_len) -> slot_cap
    -> [[the task's slot (a copy) per chunk] per stream], [[count per chunk] per stream], tasks"""
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
                tasks.append(YTask(stream_off=soff[i], stream_len=len(s), chunk_off=off, slot_off=sl, chunk_len=ln, slot_cap=cap, level=2, bpp=bpp,
                                   last=int(k == len(cuts) - 1), count_idx=idx, flags=flags, token_off=tk, token_cap=4 * ln))
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
    assert SL.launch(DYNAMIC, arena, obuf, tbuf, (YTask * max(len(tasks), 1))(*tasks), cbuf, len(tasks), grid, emu=_emu) == 0
    assert arena.tobytes() == before.tobytes(), "the streams were written"
    assert (obuf[:GAP] == FILL).all() and (obuf[sl:] == FILL).all(), "a sentinel around the slots was written"
    assert (tbuf[:GAP] == FILL).all() and (tbuf[tk:] == FILL).all(), "a sentinel around the token rows was written"
    assert (cfull[:GAP + 4] == FILL).all() and (cbuf[4 * idx:] == FILL).all(), "a sentinel around the counts was written"
    counts = cbuf[: 4 * idx].view(np.uint32)
    assert (counts[idx - 3:] == PATTERN32).all()
    out, cnt = [], []
    for i, w in enumerate(where):
        for k, (o, cap, _, t, tcap) in enumerate(w):
            assert (obuf[o + cap: o + cap + 16] == FILL).all(), "the bytes behind a slot were written"
            assert (tbuf[t + tcap: t + tcap + 16] == FILL).all(), "the bytes behind a token row were written"
            if keep is not None and not keep(i, k):
                assert (tbuf[t: t + tcap] == FILL).all(), "the token row of a task that is not in the launch was written"
        out.append([obuf[o: o + cap].copy() for o, cap, _, _, _ in w])
        cnt.append([int(counts[j]) for _, _, j, _, _ in w])
    return out, cnt, tasks


def level1(streams, bpp, flags):
    """the level-1 kernel's bytes per task, once through the same seam"""
    out, cnt, _ = E.run_deflate(streams, 1, bpp, flags=flags)
    return [[o[:c].tobytes() for o, c in zip(os_, cs)] for os_, cs in zip(out, cnt)]


def check_dynamic(streams, bpp=1, flags=0, keep=None, caps=None):
    """-> [[(the task's bytes, what the restated choice says) per chunk] per stream], after every check the module's docstring lists"""
    runs = [run_dynamic(streams, bpp, grid=g, reverse=r, flags=flags, keep=keep, caps=caps) for g, r in ((0, False), (1, True), (3, False), (0, False))]
    out, cnt, _ = runs[0]
    tokens1 = level1(streams, bpp, R.NO_STORED)
    bytes1 = level1(streams, bpp, flags & R.NO_STORED)
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
            tokens = D.tokens_of(tokens1[i][k])
            assert D.expand(tokens, s[:off]) == s[off: off + ln]
            what = D.choice(tokens, ln, last, flags, None if caps is None else caps(ln))
            want = D.dynamic_block(tokens, last) if what == "dynamic" else bytes1[i][k]
            assert data == want, (i, k, what, len(data), len(want))
            blks = D.blocks(data)
            assert blks[0]["btype"] == {"dynamic": 2, "fixed": 1, "stored": 0}[what]
            assert [b["final"] for b in blks] == [0] * (len(blks) - 1) + [int(last)]
            if not flags:
                assert n <= len(bytes1[i][k]) <= 5 + ln + (0 if last else 5)
            res[i].append((data, what))
    return res


def _whats(res):
    return [w for r in res for _, w in r]


# ---- the dynamic kernel ------------------------------------------------------------------------------------------------------------


def _text(n, seed=None):
    rng = np.random.default_rng(n if seed is None else seed)
    return np.repeat(rng.integers(0, 40, n // 3 + 1), 3)[:n].astype(np.uint8).tobytes()  # triples: short matches everywhere


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_chunk_lengths(n):
    res = check_dynamic([_text(n)], bpp=3)
    assert E.zlib_inflate(b"".join(d for d, _ in res[0])) == _text(n)
    if n >= 63:
        assert _whats(res)[0] == "dynamic"


def test_600_equal_bytes_use_one_distance_symbol():
    (data, what), = check_dynamic([bytes([7]) * 600], flags=D.ONLY_DYNAMIC)[0]
    b = D.blocks(data)[0]
    assert what == "dynamic" and b["hdist"] == 2 and b["d_lens"][:2] == [1, 1] and {d for _, d in b["matches"]} == {1}
    check_dynamic([bytes([7]) * 600])


def test_all_256_values_once_give_flat_lengths_and_symbol_16():
    (data, what), = check_dynamic([bytes(range(256))], flags=D.ONLY_DYNAMIC)[0]
    b = D.blocks(data)[0]
    assert what == "dynamic" and not b["matches"] and b["d_lens"][:2] == [1, 1] and 16 in {s for s, _ in b["hdr"]}
    assert set(b["ll_lens"][:257]) <= {8, 9}
    check_dynamic([bytes(range(256))])


def test_two_values_give_long_zero_runs_in_the_header():
    rng = np.random.default_rng(6)
    s = (rng.integers(0, 2, 3000) * 199 + 3).astype(np.uint8).tobytes()  # the values 3 and 202: 198 zeros between them, 138 + 60
    (data, what), = check_dynamic([s])[0]
    hdr = D.blocks(data)[0]["hdr"]
    assert what == "dynamic" and (18, 127) in hdr and 17 in {h for h, _ in hdr} and sum(h == 18 for h, _ in hdr) >= 2


def test_a_run_across_a_chunk_seam():
    rng = np.random.default_rng(1)
    noise = rng.integers(0, 64, CHUNK - 100, dtype=np.uint8).tobytes()
    res = check_dynamic([noise + bytes([9]) * 400 + noise[:50]])
    assert D.blocks(res[0][1][0])[0]["matches"][0] == (258, 1)  # the second chunk starts inside the run


@pytest.mark.parametrize("period", [32768, 32769])
def test_the_window_edge(period):
    block = np.random.default_rng(period).integers(0, 64, period, dtype=np.uint8).tobytes()
    res = check_dynamic([block * 2, block[:300] + bytes(period - 300) + block[:300] + b"end"])
    assert all(d <= 32768 for r in res for t, _ in r for b in D.blocks(t) for _, d in b["matches"])
    m = D.blocks(res[1][1][0])[0]["matches"]
    assert m[0] == (258, 32768) if period == 32768 else all(d < 300 for _, d in m)


def far_copy_stream():
    """a chunk of six-bit noise in front; a second one of six-bit noise with three hundred short copies from nearby and ONE copy of
    200 bytes from 20 000 back: its length symbol and its distance symbol are rare, so both codes are long"""
    rng = np.random.default_rng(77)
    s = bytearray(rng.integers(0, 64, 2 * CHUNK, dtype=np.uint8).tobytes())
    for k in range(300):
        at = CHUNK + 100 + 100 * k
        d = int(rng.integers(1, 400))
        ln = int(rng.integers(5, 9))
        s[at: at + ln] = s[at - d: at - d + ln]
    at = CHUNK + 31000
    s[at: at + 200] = s[at - 20000: at - 20000 + 200]
    return bytes(s)


def test_a_token_of_more_than_32_bits():
    res = check_dynamic([far_copy_stream()])
    data, what = res[0][1]
    b = D.blocks(data)[0]
    far = [ln for ln, d in b["matches"] if d == 20000]
    assert what == "dynamic" and b["bits"] >= 32 and max(far) >= 100, (b["bits"], far)


@pytest.mark.parametrize("n", [1, 2, 5, 40, 300])
def test_only_dynamic_on_small_chunks(n):
    s = bytes(range(200, 200 + n)) if n < 50 else np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    for stream in (s, _text(CHUNK) + s):  # as a last chunk, and a first chunk in front of it
        res = check_dynamic([stream], flags=D.ONLY_DYNAMIC)
        assert all(w == "dynamic" and D.blocks(d)[0]["btype"] == 2 for d, w in res[0])


def test_only_dynamic_that_does_not_fit():
    """n different bytes: from some n on the header of the dynamic block makes it longer than the worst-case slot, which is sized for
    stored and fixed blocks; the task then writes what level 1 writes.  A long chunk's dynamic block always fits."""
    noise = np.random.default_rng(2).integers(0, 256, 3000, dtype=np.uint8).tobytes()
    assert _whats(check_dynamic([noise], flags=D.ONLY_DYNAMIC)) == ["dynamic"]
    for n in range(20, 60):
        s = bytes(range(255, 255 - 4 * n, -4))
        if (D.block_bytes(D.sizes(list(s), n, True)[2], True) + 3) // 4 * 4 > R.slot_bytes(n):
            break
    else:
        pytest.fail("no input whose dynamic block is longer than its slot")
    assert _whats(check_dynamic([s], flags=D.ONLY_DYNAMIC)) == ["stored"]
    assert _whats(check_dynamic([s], flags=D.ONLY_DYNAMIC | R.NO_STORED)) == ["fixed"]
    assert _whats(check_dynamic([s], flags=D.ONLY_DYNAMIC, caps=lambda ln: R.slot_bytes(ln) + 64)) == ["dynamic"]  # the same in a larger slot


def test_the_choice_takes_every_branch():
    noise = np.random.default_rng(3).integers(0, 256, CHUNK + 700, dtype=np.uint8).tobytes()
    res = check_dynamic([noise, bytes(2 * CHUNK + 77), bytes([200, 201, 202]), _text(5000)])
    w = _whats(res)
    assert "stored" in w and "fixed" in w and "dynamic" in w
    check_dynamic([noise[:2000], bytes([200, 201, 202])], flags=R.NO_STORED)


def test_tasks_not_in_the_launch_keep_their_slots_and_rows():
    s = _text(2 * CHUNK + 500, 3)
    check_dynamic([s, s[:100], s[5:]], bpp=3, keep=lambda i, k: (i + k) % 2 == 0)


def test_tasks_that_break_a_bound_dynamic():
    s = _text(1500, 4)
    edits = [("chunk_len", 0), ("chunk_off", 1500), ("chunk_len", 1501), ("slot_cap", R.slot_bytes(1500) - 16), ("level", 1), ("level", 3),
             ("last", 2), ("bpp", 0), ("bpp", 9), ("chunk_len", CHUNK + 1), ("slot_off", None), ("token_off", None), ("token_cap", 4 * 1500 - 1)]
    streams = [s] * (len(edits) + 1)

    def spoil(tasks):
        for k, (field, v) in enumerate(edits):
            setattr(tasks[k], field, getattr(tasks[k], field) + 2 if v is None else v)

    out, cnt, _ = run_dynamic(streams, spoil=spoil, keep=lambda i, k: True)
    for k in range(len(edits)):
        assert cnt[k][0] == PATTERN32 and (out[k][0] == FILL).all(), (k, edits[k])
    R.check_task(out[len(edits)][0][: cnt[len(edits)][0]].tobytes(), 0, s)


# ---- the code builder --------------------------------------------------------------------------------------------------------------


def run_codes(cases, grid=0, reverse=False, spoil=None):
    """cases: [(counts, limit)] -> [the n length bytes per case (a copy)]"""
    coff, loff, at, lt = [], [], 4, GAP
    for counts, _ in cases:
        coff.append(at)
        at += 4 * len(counts) + 4
        lt += 1
        loff.append(lt)
        lt += len(counts)
    cbuf = E._aligned(at + 16, 0x5A)
    for (counts, _), o in zip(cases, coff):
        cbuf[o: o + 4 * len(counts)] = np.asarray(counts, np.uint32).view(np.uint8)
    before = cbuf.copy()
    lbuf = E._aligned(lt + GAP, FILL)
    tasks = [CTask(counts_off=co, lens_off=lo, n=len(c), limit=lim) for (c, lim), co, lo in zip(cases, coff, loff)]
    if spoil:
        spoil(tasks)
    if reverse:
        tasks = tasks[::-1]
    assert SL.launch(CODES, cbuf, lbuf, (CTask * max(len(tasks), 1))(*tasks), len(tasks), grid, emu=_emu) == 0
    assert cbuf.tobytes() == before.tobytes(), "the counts were written"
    assert (lbuf[:GAP] == FILL).all() and (lbuf[lt:] == FILL).all(), "a sentinel around the lengths was written"
    at = GAP
    for (counts, _), o in zip(cases, loff):
        assert (lbuf[at: o] == FILL).all(), "the byte between two length lists was written"
        at = o + len(counts)
    return [lbuf[o: o + len(c)].copy() for (c, _), o in zip(cases, loff)]


def check_codes(cases):
    runs = [run_codes(cases, grid=g, reverse=r) for g, r in ((0, False), (1, True), (3, False))]
    for k, (counts, limit) in enumerate(cases):
        want = D.code_lengths(list(counts), limit)
        for run in runs:
            assert run[k].tolist() == want, (k, limit, list(counts)[:20])
    return runs[0]


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def test_codes_fibonacci_counts_drive_the_limiter():
    a, b = fib(20), fib(10)
    assert sum(a) == 17710 and max(D.tree_depths(a)[1]) == 19 > 15 and max(D.tree_depths(b)[1]) == 9 > 7
    got = check_codes([(a, 15), (b, 7), (a[::-1], 15), ([0, 0] + b + [0], 7)])
    assert got[0].max() == 15 and got[1].max() == 7 and D.kraft(got[0].tolist(), 15) == 1 << 15 and D.kraft(got[1].tolist(), 7) == 1 << 7


def test_codes_flat_sparse_and_large_counts():
    far = [0] * 286
    far[0], far[285] = 5, 9
    one = [0] * 30
    one[17] = 4
    got = check_codes([([7] * 286, 15), (one, 15), ([0] * 30, 15), ([0] * 19, 7), (far, 15), ([32768] * 286, 15), ([32768] * 19, 7), ([3], 1), ([0, 1], 1),
                       ([MAX_COUNT] * 286, 15), ([1, 1, 1], 2)])
    assert set(got[0].tolist()) == {8, 9} and got[1].tolist() == [1] + [0] * 16 + [1] + [0] * 12 and got[2].tolist() == [1, 1] + [0] * 28
    assert got[4][0] == 1 and got[4][285] == 1 and got[4].sum() == 2


def test_codes_random_histograms():
    rng = np.random.default_rng(20261021)
    cases = []
    for k in range(60):
        n, limit = [(286, 15), (30, 15), (19, 7)][k % 3]
        kind = k % 4
        c = rng.integers(0, 1 << int(rng.integers(1, 16)), n)
        if kind == 1:
            c = (rng.pareto(0.7, n) * 3).astype(np.int64).clip(0, 32768)  # skewed: deep trees
        elif kind == 2:
            c = c * (rng.integers(0, 4, n) == 0)  # sparse
        elif kind == 3:
            c = rng.integers(0, 3, n)  # ties everywhere
        cases.append((c.astype(np.uint32).tolist(), limit))
    got = check_codes(cases)
    for (c, limit), g in zip(cases, got):
        if sum(1 for v in c if v) >= 2:
            assert D.kraft(g.tolist(), limit) == 1 << limit and g.max() <= limit


def test_tasks_that_break_a_bound_codes():
    good = list(range(1, 31))
    edits = [("n", 0), ("n", 287), ("limit", 0), ("limit", 16), ("limit", 4), ("counts_off", None), ("n", 30)]
    cases = [(good, 15)] * (len(edits) + 1)
    big = good[:]
    big[11] = MAX_COUNT + 1
    cases[6] = (big, 15)

    def spoil(tasks):
        for k, (field, v) in enumerate(edits):
            setattr(tasks[k], field, getattr(tasks[k], field) + 2 if v is None else v)

    got = run_codes(cases, spoil=spoil, grid=2)
    for k in range(len(edits)):
        assert (got[k] == FILL).all(), (k, edits[k])
    assert got[len(edits)].tolist() == D.code_lengths(good, 15)


# ---- whole files from the kernels: what tests/golden/png_encode_dyn.json records -----------------------------------------------------

def golden_inputs():
    """the seeded inputs of tests/test_emu_png_encode.py at level 2, and two label maps large enough for several chunks"""
    rng = np.random.default_rng(20261022)
    cases = [(name, im, filt, pal, trns) for name, im, filt, level, pal, trns in E.golden_inputs() if level == 1]
    pal = rng.integers(0, 256, (21, 3), dtype=np.uint8)
    blocky = np.repeat(np.repeat(rng.integers(0, 21, (20, 25, 1)), 13, axis=0), 11, axis=1)  # 260 x 275: three chunks
    ids = np.repeat(np.repeat(rng.integers(0, 3000, (12, 9, 1)), 9, axis=0), 11, axis=1)
    return cases + [("blocky_three_chunks_none", E.Img(blocky, palette=21), 0, pal, None),
                    ("blocky_three_chunks_adaptive", E.Img(blocky, "int32", 8, palette=21), 5, pal, None),
                    ("ids_uint16_none", E.Img(ids, "uint16"), 0, None, None)]


def kernels_file(im, filt, palette=None, trns=None):
    """one level-2 PNG file from the filter and the dynamic kernel through the launch seam, the container, the zlib header and the two
    checksums from the restatement and zlib"""
    import zlib

    streams, flags, _, _ = E.run_filter([im], filt)
    assert flags[0] == 0
    stream = streams[0].tobytes()
    out, cnt, _ = run_dynamic([stream], bpp=im.C * im.depth // 8)
    payload = b"".join(o[:c].tobytes() for o, c in zip(out[0], cnt[0]))
    zdata = b"\x78\x5e" + payload + (zlib.adler32(stream) & 0xFFFFFFFF).to_bytes(4, "big")
    return R.container(im.W, im.H, im.C, im.depth, zdata, palette, trns)


def golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_encode_dyn.json")


def test_the_recorded_digests_are_those_of_the_emulator_path():
    rec = json.load(open(golden_path()))
    cases = golden_inputs()
    assert sorted(rec) == sorted(c[0] for c in cases) and len(cases) >= 12
    for name, im, filt, pal, trns in cases:
        data = kernels_file(im, filt, pal, trns)
        assert hashlib.sha256(data).hexdigest() == rec[name], name
        st, got, inf, _, _ = R.samples_of(data)
        assert st == 0 and np.array_equal(got, im.s), name
