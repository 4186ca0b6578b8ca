"""What of level 2 of the PNG encode (include/decode_png.h: debig_png_encode_batch_dyn) can be checked without a device:
  * the restated rule of tests/png_encode_dyn_ref.py on its own terms: every code complete (Kraft sum exactly 2^L), within the limit
    and monotone in the count, on random histograms, on Fibonacci counts (limiter active) and on the small cases of the rule's
    first step; canonical codes that are prefix free; the header rule on lists made by hand;
  * zlib inflates dynamic_block() of hand-made token lists to the bytes the tokens stand for; the bit reader reads them back; the
    three sizes are the blocks' sizes; the choice;
  * the argument rules of the C call that are decided before any device work, the ValueErrors of api.png_encode_batch_dyn, the new
    symbols and constants;
  * the stand-alone sanitizer program, as a plain child process."""
import ctypes as C
import inspect
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_dyn_ref as D  # noqa: E402
import png_encode_ref as R  # noqa: E402
from test_png_encode_cpu import DUMMY, GOOD, BAD_DESCS, Desc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    from debigulator_amd import api as A_

    return A_


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    for name in ("debig_png_encode_batch", "debig_png_encode_batch_dyn"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p] * 7 + [C.c_uint32] * 3
    return L


# ---- the rule ----------------------------------------------------------------------------------------------------------------------

def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def check_code(counts, limit):
    lens = D.code_lengths(counts, limit)
    used = [s for s, c in enumerate(counts) if c]
    assert len(lens) == len(counts) and all(0 <= l <= limit for l in lens)
    if len(used) >= 2:
        assert all((lens[s] > 0) == (counts[s] > 0) for s in range(len(counts)))
    assert D.kraft(lens, limit) == 1 << limit or len(counts) < 2, (counts, lens)
    for a in used:  # monotone: a larger count never has a longer code
        for b in used:
            assert not (counts[a] > counts[b] and lens[a] > lens[b]), (a, b)
    codes = D.canonical(lens)
    words = sorted(format(c, "0%db" % l) for l, c in zip(lens, codes) if l)
    assert all(not y.startswith(x) for x, y in zip(words, words[1:])), "the canonical code is not prefix free"
    return lens


def test_random_histograms_are_complete_limited_and_monotone():
    rng = np.random.default_rng(1951)
    for k in range(300):
        n, limit = [(286, 15), (30, 15), (19, 7)][k % 3]
        c = rng.integers(0, 1 << int(rng.integers(1, 16)), n)
        if k % 4 == 1:
            c = (rng.pareto(0.7, n) * 3).astype(np.int64).clip(0, 32768)
        elif k % 4 == 2:
            c = c * (rng.integers(0, 4, n) == 0)
        check_code([int(v) for v in c], limit)


def test_fibonacci_counts_drive_the_limiter():
    a, b = fib(20), fib(10)
    assert sum(a) == 17710 <= R.CHUNK and max(D.tree_depths(a)[1]) == 19 and max(D.tree_depths(b)[1]) == 9
    la, lb = check_code(a, 15), check_code(b, 7)
    assert max(la) == 15 and max(lb) == 7
    assert check_code(a, 19) == [19, 19] + list(range(18, 0, -1))  # not limited: the tree's own depths
    assert check_code([0, 0] + b[::-1] + [0], 7)[2:12] == lb[::-1]  # a tie is broken by the index, so only mirrored counts mirror


def test_the_first_step_of_the_rule():
    assert D.code_lengths([0] * 30, 15) == [1, 1] + [0] * 28  # a chunk without matches
    one = [0] * 30
    one[0] = 9
    assert D.code_lengths(one, 15) == [1, 1] + [0] * 28
    one = [0] * 30
    one[5] = 9
    assert D.code_lengths(one, 15) == [1] + [0] * 4 + [1] + [0] * 24
    far = [0] * 286
    far[0], far[285] = 5, 9
    assert D.code_lengths(far, 15) == [1] + [0] * 284 + [1]
    assert set(D.code_lengths([7] * 286, 15)) == {8, 9} and D.code_lengths([7] * 256, 15) == [8] * 256
    assert D.code_lengths([32768] * 19, 7) == [5] * 6 + [4] * 13  # 6 x 2^-5 + 13 x 2^-4 = 1; the order's first symbols are the longest
    # ties go to the lower index first in the order, so the LOWER index gets the longer code
    assert D.code_lengths([1, 1, 1], 15) == [2, 2, 1]
    assert D.canonical([2, 1, 3, 3]) == [0b10, 0b0, 0b110, 0b111]  # RFC 1951 3.2.2's procedure


def test_the_header_rule_on_lists_made_by_hand():
    ll = [0] * 286
    ll[3], ll[202], ll[256] = 1, 2, 2
    hlit, hdist, hdr = D.header_symbols(ll, [1, 1] + [0] * 28)
    assert (hlit, hdist) == (257, 2)
    # 3 zeros (17), 1, 198 zeros (18 for 138, 18 for 60), 2, 53 zeros (18), 2; then 1, 1 of the distance code
    assert hdr == [(17, 0), (1, 0), (18, 127), (18, 49), (2, 0), (18, 42), (2, 0), (1, 0), (1, 0)]
    flat = [8] * 286
    hlit, hdist, hdr = D.header_symbols(flat, [5] * 30)
    assert (hlit, hdist) == (286, 30) and hdr[:3] == [(8, 0), (16, 3), (16, 3)]
    assert hdr == [(8, 0)] + [(16, 3)] * 47 + [(16, 0)] + [(5, 0)] + [(16, 3)] * 4 + [(16, 2)]  # 285 = 47 x 6 + 3; 29 = 4 x 6 + 5
    # a run crosses the seam between the two lists, a rest of 1 .. 2 is written out, 139 zeros are 138 + one zero
    ll = [0] * 286
    ll[0], ll[140], ll[255], ll[256] = 3, 3, 4, 4
    hlit, hdist, hdr = D.header_symbols(ll, [4, 4, 0, 0, 7] + [0] * 25)
    assert hdr == [(3, 0), (18, 127), (0, 0), (3, 0), (18, 103), (4, 0), (16, 0), (0, 0), (0, 0), (7, 0)] and (hlit, hdist) == (257, 5)


# ---- the block ---------------------------------------------------------------------------------------------------------------------

HAND = [
    [65],
    [0, 255, 0, 255, (4, 2)],
    [7, (258, 1), (258, 1), (83, 1)],
    list(range(256)),
    list(b"abcabcabd") + [(6, 9), (3, 3), (258, 6), 200, (5, 24)],
    [1, 2, 3, 4] * 10 + [(3, 1), (4, 2), (10, 3), (11, 4), (18, 5), (19, 7), (35, 9), (67, 13), (131, 17), (227, 25), (257, 33), (258, 40)],
]


@pytest.mark.parametrize("k", range(len(HAND)))
@pytest.mark.parametrize("last", [1, 0])
def test_zlib_inflates_the_restated_dynamic_block(k, last):
    tokens = HAND[k]
    want = D.expand(tokens)
    data = D.dynamic_block(tokens, last)
    d = zlib.decompressobj(-15)
    assert d.decompress(data) == want and d.eof == bool(last) and d.unused_data == b""
    if not last:
        assert data[-4:] == b"\x00\x00\xff\xff"
    blks = D.blocks(data)
    p = D.plan(tokens)
    b = blks[0]
    assert b["btype"] == 2 and b["final"] == last and b["tokens"] == tokens and b["bytes"] == len(want)
    assert (b["ll_lens"], b["d_lens"], b["cl_lens"], b["hlit"], b["hdist"], b["hclen"], b["hdr"]) == \
        (p["ll_lens"], p["d_lens"], p["cl_lens"], p["hlit"], p["hdist"], p["hclen"], p["hdr"])
    stored, fixed, dyn = D.sizes(tokens, len(want), last)
    assert b["end"] == dyn and len(data) == D.block_bytes(dyn, last) and stored == 5 + len(want) + (0 if last else 5)
    assert D.kraft(b["cl_lens"], 7) == 1 << 7 and max(b["cl_lens"]) <= 7 and 4 <= b["hclen"] <= 19


def test_a_far_long_match_among_many_symbols_has_more_than_32_bits():
    rng = np.random.default_rng(5)
    tokens = [int(v) for v in rng.integers(0, 256, 4000)] + [(4 + k % 5, 1 + k % 300) for k in range(400)] + [(200, 20000)]
    data = D.dynamic_block(tokens, 1)
    b = D.blocks(data)[0]
    assert b["tokens"] == tokens and b["bits"] >= 32
    pre = bytes(rng.integers(0, 256, 20000, dtype=np.uint8))
    assert zlib.decompressobj(-15, zdict=pre).decompress(data) == D.expand(tokens, pre)


def test_the_choice():
    text = [int(v) for v in np.random.default_rng(3).integers(0, 30, 5000)]
    assert D.choice(text, 5000, True) == "dynamic"
    noise = [int(v) for v in np.random.default_rng(4).integers(0, 256, 5000)]
    assert D.choice(noise, 5000, True) == "stored" and D.choice(noise, 5000, True, R.NO_STORED) in ("fixed", "dynamic")
    assert D.choice([200, 201, 202], 3, True) == "fixed" and D.choice([1, 2, 3], 3, True, R.NO_STORED) == "fixed"  # 37 bits against 8 bytes
    assert D.choice([1, 2, 3], 3, True, D.ONLY_DYNAMIC) == "dynamic"
    zeros = [0, (258, 1)]
    stored, fixed, dyn = D.sizes(zeros, 259, True)
    assert fixed == 3 + 8 + 8 + 5 + 7 and fixed < dyn and D.choice(zeros, 259, True) == "fixed"  # two tokens: a header costs more than it saves
    many = list(range(255, 255 - 4 * 57, -4))  # 57 different bytes: a dynamic block of 98 bytes, a slot of 96
    assert D.block_bytes(D.sizes(many, 57, True)[2], True) == 98 and R.slot_bytes(57) == 96
    assert D.choice(many, 57, True, D.ONLY_DYNAMIC) == "stored" and D.choice(many, 57, True, D.ONLY_DYNAMIC | R.NO_STORED) == "fixed"
    assert D.choice(many, 57, True, D.ONLY_DYNAMIC, slot_cap=256) == "dynamic"


# ---- the C call and Python ---------------------------------------------------------------------------------------------------------

def _call(lib, descs, ptrs, filt=5, level=2, side=b"\0" * 2048, outs=True):
    n = len(descs)
    arr = (Desc * n)(*[Desc(**d) for d in descs])
    bufs = [(C.c_uint8 * 64)(*([0xAB] * 64)) for _ in range(n)]
    sizes, status = (C.c_uint64 * n)(*([77] * n)), (C.c_uint32 * n)(*([99] * n))
    rc = lib.debig_png_encode_batch_dyn((C.c_void_p * n)(*ptrs) if ptrs is not None else None, arr, side,
                                        (C.c_void_p * n)(*[C.addressof(b) for b in bufs]) if outs else None, (C.c_uint64 * n)(*([64] * n)), sizes,
                                        status, n, filt, level)
    assert all(bytes(b) == b"\xab" * 64 for b in bufs)
    return rc, list(status), list(sizes)


def test_c_argument_checks_come_before_any_device_work(lib):
    for kw in (dict(ptrs=None), dict(outs=False), dict(filt=6), dict(level=3), dict(level=2 ** 32 - 1)):
        rc, status, sizes = _call(lib, [GOOD, GOOD], kw.pop("ptrs", [DUMMY, DUMMY]), **kw)
        assert rc == R.BAD_ARG and status == [99, 99] and sizes == [77, 77], kw
    rc, status, _ = _call(lib, [dict(GOOD, channels=1, palette_entries=4)], [DUMMY], side=None)
    assert rc == R.BAD_ARG and status == [99]
    assert lib.debig_png_encode_batch_dyn(None, None, None, None, None, None, None, 0, 9, 9) == 0
    # a batch of bad descriptors only is decided on the host at every level; the old call still refuses level 2
    descs = [dict(GOOD, **b) for b in BAD_DESCS]
    for level in (0, 1, 2):
        rc, status, sizes = _call(lib, descs, [DUMMY] * len(descs), level=level)
        assert rc == 0 and status == [R.E_ENCODE] * len(descs) and sizes == [0] * len(descs)
    n = 1
    assert lib.debig_png_encode_batch((C.c_void_p * n)(DUMMY), (Desc * n)(Desc(**GOOD)), None, (C.c_void_p * n)(), (C.c_uint64 * n)(),
                                      (C.c_uint64 * n)(), (C.c_uint32 * n)(), n, 5, 2) == R.BAD_ARG


def test_symbols_constants_and_documents(lib, api):
    for name in ("debig_png_encode_batch_dyn", "debig_hip_png_encode_dynamic_batch", "debig_hip_png_encode_codes_batch"):
        assert hasattr(lib, name), name
    pub = open(os.path.join(ROOT, "include", "decode_png.h")).read()
    dev = open(os.path.join(ROOT, "include", "debig_hip.h")).read()
    for text in ("int debig_png_encode_batch_dyn(", "78 5E", "dynamic Huffman blocks, lazy matching, levels above 1"):
        assert text in pub, text
    for text in ("#define DEBIG_PNG_ENCODE_ONLY_DYNAMIC %du" % D.ONLY_DYNAMIC, "#define DEBIG_PNG_ENCODE_ROUND_TASKS %du" % D.ROUND_TASKS,
                 "} debig_png_encode_dynamic_task;", "} debig_png_encode_codes_task;", "#define DEBIG_PNG_ENCODE_CODES_MAX_COUNT (1u << 22)"):
        assert text in dev, text
    assert D.ROUND_TASKS * 4 * R.CHUNK == 256 << 20
    emu = open(os.path.join(ROOT, "tools", "simt_emu", "emu_lib.cpp")).read()
    assert "emu_png_encode_dynamic_batch" in emu and "emu_png_encode_codes_batch" in emu


def test_png_encode_batch_dyn_argument_rules(api):
    import torch

    ok = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    for level in (0, 1, 2):
        with pytest.raises(ValueError, match="GPU"):
            api.png_encode_batch_dyn(ok, level=level)
    for lv in (3, -1, "2", None, True, 9):
        with pytest.raises(ValueError, match="level must be 0, 1 or 2"):
            api.png_encode_batch_dyn(ok, level=lv)
    with pytest.raises(ValueError, match="level must be 0 or 1"):
        api.png_encode_batch(ok, level=2)
    with pytest.raises(ValueError, match="filter"):
        api.png_encode_batch_dyn(ok, filter="best")
    with pytest.raises(ValueError, match="depth"):
        api.png_encode_batch_dyn(ok, depth=4)
    with pytest.raises(ValueError, match="layout"):
        api.png_encode_batch_dyn(ok, layout="nhwc")
    with pytest.raises(ValueError, match="uint8, uint16"):
        api.png_encode_batch_dyn(torch.zeros((2, 4, 5), dtype=torch.float32))
    with pytest.raises(ValueError, match="tensor"):
        api.png_encode_batch_dyn(None)
    with pytest.raises(ValueError, match="palette must"):
        api.png_encode_batch_dyn(ok[..., 0], palette=np.zeros((4, 4), np.uint8))
    assert api.png_encode_batch_dyn([]) == [] and api.png_encode_batch_dyn(ok[:0]) == []
    sig, old = inspect.signature(api.png_encode_batch_dyn), inspect.signature(api.png_encode_batch)
    assert list(sig.parameters) == list(old.parameters) == ["images", "layout", "depth", "palette", "trns", "filter", "level"]
    assert [p.default for p in sig.parameters.values()][1:] == ["hwc", None, None, None, "adaptive", 2]


# ---- the sanitizer program (stand-alone, a plain child process) --------------------------------------------------------------------

def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    import subprocess

    r = subprocess.run(["sh", os.path.join(ROOT, "tools", "asan_png_encode_dyn_emu.sh"), str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
