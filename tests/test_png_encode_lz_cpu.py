"""What of level 3 of the PNG encode (include/decode_png.h: debig_png_encode_batch_lz) can be checked without a device:
  * the restated rule of tests/png_encode_lz_ref.py on its own terms: the tokens expand to the chunk, zlib inflates fixed_block() and
    the stored block, hand-made streams give the lengths, candidates and deferrals the rule's words say;
  * the issue's two label maps through the restatement alone: the DEFLATE bytes of its table;
  * the argument rules of the C call that are decided before any device work, the ValueErrors of api.png_encode_batch_lz, the new
    symbols, and that the two older calls still refuse level 3;
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
import png_encode_lz_ref as Z  # noqa: E402
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
    for name in ("debig_png_encode_batch", "debig_png_encode_batch_dyn", "debig_png_encode_batch_lz"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p] * 7 + [C.c_uint32] * 3
    return L


# ---- the rule ----------------------------------------------------------------------------------------------------------------------

def test_the_fixed_distances_and_the_stride_rule():
    assert Z.fixed_distances(1, 0) == [1] and Z.fixed_distances(3, 0) == [1, 3]
    assert Z.fixed_distances(1, 401) == [1, 401, 400, 402] and Z.fixed_distances(3, 1201) == [1, 3, 1201, 1198, 1204]
    assert Z.fixed_distances(3, 4) == [1, 3, 4, 7] and Z.fixed_distances(2, 4) == [1, 2, 4, 6] and Z.fixed_distances(1, 2) == [1, 2, 3]
    assert Z.stride_ok(3, 0) and Z.stride_ok(3, 4) and not Z.stride_ok(3, 3) and Z.stride_ok(3, 32765) and not Z.stride_ok(3, 32766)
    assert Z.host_stride(400, 1, 8) == 401 and Z.host_stride(16384, 1, 8) == 16385 and Z.host_stride(16384, 1, 16) == 0
    assert Z.host_stride(8190, 4, 8) == 32761 and Z.host_stride(8191, 4, 8) == 0  # 32765 + 4 > 32768


def test_lengths_on_streams_made_by_hand():
    # two rows of ten different bytes: the second row matches the first at S = 10, the table's candidate is the same distance
    row = bytes(range(50, 60))
    L, d = Z.lengths(row * 2, 0, 20, 1, 10)
    assert L.tolist() == [0] * 10 + [10, 9, 8, 7, 6, 5, 4, 3, 0, 0] and set(d[10:18].tolist()) == {10}
    # without the stride nothing matches: the first row is in the same step, so the table does not hold it yet
    L0, d0 = Z.lengths(row * 2, 0, 20, 1, 0)
    assert not L0.any() and not d0.any()
    # ... and it does once the first row lies a step back
    L0, d0 = Z.lengths(bytes(range(100, 154)) + row * 2, 0, 74, 1, 0)
    assert L0[64:74].tolist() == [10, 9, 8, 7, 6, 5, 4, 3, 0, 0] and set(d0[64:72].tolist()) == {10}
    # a run: distance 1 wins every tie, the last two positions have fewer than three bytes left
    L, d = Z.lengths(bytes([4]) * 300, 0, 300, 2, 7)
    assert L[0] == 0 and L[1:43].tolist() == [258] * 42 and L[297] == 3 and L[298] == 0 and set(d[1:298].tolist()) == {1}
    # a chunk in the middle of a stream: the row above lies in front of the chunk, the match stops at the chunk's end
    s = bytes(range(100)) * 3
    L, d = Z.lengths(s, 150, 100, 1, 100)
    assert L[0] == 100 and d[0] == 100 and L[97] == 3 and L[98] == 0
    # a match of three bytes farther than 4096 is no match
    rng = np.random.default_rng(1)
    far = bytes([200, 201, 202]) + rng.integers(0, 128, 5000, dtype=np.uint8).tobytes() + bytes([200, 201, 202, 203])
    L, d = Z.lengths(far, 0, len(far), 1, 0)
    assert L[5003] == 0
    L, d = Z.lengths(far, 0, len(far), 1, 5003 - 0)  # the same distance as S: still three bytes, still too far
    assert L[5003] == 0


def test_the_walk_defers_once_per_position():
    L = np.zeros(200, np.int64)
    dist = np.ones(200, np.int64)
    L[10], L[11] = 4, 6  # defers
    L[30], L[31] = 4, 4  # not longer: taken
    L[62], L[63], L[64] = 3, 5, 9  # 62 defers, 63 never does
    L[100], L[101] = 16, 30  # 16 is not below max_lazy
    L[120], L[121] = 15, 30
    s = bytes(200)
    tokens, deferred = Z.walk(s, 0, 200, L, dist)
    assert deferred == [10, 62, 120]
    starts = np.cumsum([0] + [t[0] if isinstance(t, tuple) else 1 for t in tokens]).tolist()
    assert tokens[starts.index(11)] == (6, 1) and tokens[starts.index(30)] == (4, 1) and tokens[starts.index(63)] == (5, 1)
    assert tokens[starts.index(100)] == (16, 1) and tokens[starts.index(121)] == (30, 1) and starts[-1] == 200
    # the last position of the chunk has no neighbour
    L = np.zeros(5, np.int64)
    tokens, deferred = Z.walk(bytes(5), 0, 5, L, L)
    assert tokens == [0] * 5 and not deferred


@pytest.mark.parametrize("last", [1, 0])
def test_zlib_inflates_the_restated_fixed_and_stored_blocks(last):
    rng = np.random.default_rng(8)
    s = np.repeat(rng.integers(0, 256, 700), 3).astype(np.uint8).tobytes()
    tokens = Z.tokens(s, 0, len(s), 1, 50)
    assert D.expand(tokens) == s and any(isinstance(t, tuple) for t in tokens) and any(isinstance(t, int) and t >= 144 for t in tokens)
    for data in (Z.fixed_block(tokens, last), Z.stored_block(s, last)):
        d = zlib.decompressobj(-15)
        assert d.decompress(data) == s and d.eof == bool(last) and d.unused_data == b""
        if not last:
            assert data[-4:] == b"\x00\x00\xff\xff"
    b = D.blocks(Z.fixed_block(tokens, last))[0]
    assert b["btype"] == 1 and b["tokens"] == tokens and b["end"] == D.sizes(tokens, len(s), last)[1]
    assert len(Z.stored_block(s, last)) == D.sizes(tokens, len(s), last)[0]
    assert Z.token_words([65, (3, 1), (258, 32768)]) == [65, 0x80000000, 0x80000000 | 255 << 16 | 32767]


def test_the_two_label_maps_of_the_issue_through_the_restatement():
    """the DEFLATE bytes of the issue's table, from the restated rule alone: 1773 and 8297 in its model"""
    import test_emu_png_encode_lz as Q

    for im, model, level1 in ((Q.blocky_map(), 1773, 4157), (Q.curved_map(), 8297, 13758)):
        stream = R.filtered_stream(im[:, :, None], 8, 0)
        cuts = R.chunks(len(stream))
        total = sum(len(Z.task_bytes(stream, off, ln, 1, Z.host_stride(im.shape[1], 1, 8), k == len(cuts) - 1)[0]) for k, (off, ln) in enumerate(cuts))
        print(im.shape, "level 3", total, "the model", model, "zlib.compress level 1 here", len(zlib.compress(stream, 1)) - 6, "in the issue", level1)
        assert total == model


# ---- the C call and Python ---------------------------------------------------------------------------------------------------------

def _call(lib, descs, ptrs, filt=5, level=3, side=b"\0" * 2048, outs=True, name="debig_png_encode_batch_lz"):
    n = len(descs)
    arr = (Desc * n)(*[Desc(**d) for d in descs])
    bufs = [(C.c_uint8 * 64)(*([0xAB] * 64)) for _ in range(n)]
    sizes, status = (C.c_uint64 * n)(*([77] * n)), (C.c_uint32 * n)(*([99] * n))
    rc = getattr(lib, name)((C.c_void_p * n)(*ptrs) if ptrs is not None else None, arr, side,
                            (C.c_void_p * n)(*[C.addressof(b) for b in bufs]) if outs else None, (C.c_uint64 * n)(*([64] * n)), sizes, status, n, filt,
                            level)
    assert all(bytes(b) == b"\xab" * 64 for b in bufs)
    return rc, list(status), list(sizes)


def test_c_argument_checks_come_before_any_device_work(lib):
    for kw in (dict(ptrs=None), dict(outs=False), dict(filt=6), dict(level=4), dict(level=2 ** 32 - 1)):
        rc, status, sizes = _call(lib, [GOOD, GOOD], kw.pop("ptrs", [DUMMY, DUMMY]), **kw)
        assert rc == R.BAD_ARG and status == [99, 99] and sizes == [77, 77], kw
    rc, status, _ = _call(lib, [dict(GOOD, channels=1, palette_entries=4)], [DUMMY], side=None)
    assert rc == R.BAD_ARG and status == [99]
    assert lib.debig_png_encode_batch_lz(None, None, None, None, None, None, None, 0, 9, 9) == 0
    # a batch of bad descriptors only is decided on the host at every level; the two older calls still refuse level 3
    descs = [dict(GOOD, **b) for b in BAD_DESCS]
    for level in (0, 1, 2, 3):
        rc, status, sizes = _call(lib, descs, [DUMMY] * len(descs), level=level)
        assert rc == 0 and status == [R.E_ENCODE] * len(descs) and sizes == [0] * len(descs)
    for name in ("debig_png_encode_batch", "debig_png_encode_batch_dyn"):
        rc, status, sizes = _call(lib, [GOOD], [DUMMY], level=3, name=name)
        assert rc == R.BAD_ARG and status == [99] and sizes == [77], name


def test_symbols_constants_and_documents(lib):
    for name in ("debig_png_encode_batch_lz", "debig_hip_png_encode_lz_batch"):
        assert hasattr(lib, name), name
    pub = open(os.path.join(ROOT, "include", "decode_png.h")).read()
    dev = open(os.path.join(ROOT, "include", "debig_hip.h")).read()
    for text in ("int debig_png_encode_batch_lz(", "78 9C", "NOT guaranteed to be at most level 2"):
        assert text in pub, text
    for text in ("} debig_png_encode_lz_task;", "int debig_hip_png_encode_lz_batch(", "NOT guaranteed to be at most level 2",
                 "3 <= L(q) < %d; q %% 64 != 63; q + 1 < len; L(q + 1) > L(q)" % Z.MAX_LAZY, "1. distance 1; 2. bpp, if bpp > 1; 3. S; 4. S - bpp; 5. S + bpp"):
        assert text in dev, text
    emu = open(os.path.join(ROOT, "tools", "simt_emu", "emu_lib.cpp")).read()
    assert "emu_png_encode_lz_batch" in emu


def test_png_encode_batch_lz_argument_rules(api):
    import torch

    ok = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    for level in (0, 1, 2, 3):
        with pytest.raises(ValueError, match="GPU"):
            api.png_encode_batch_lz(ok, level=level)
    for lv in (4, -1, "3", None, True, 9):
        with pytest.raises(ValueError, match="level must be 0, 1, 2 or 3"):
            api.png_encode_batch_lz(ok, level=lv)
    with pytest.raises(ValueError, match="level must be 0, 1 or 2"):
        api.png_encode_batch_dyn(ok, level=3)
    with pytest.raises(ValueError, match="filter"):
        api.png_encode_batch_lz(ok, filter="best")
    with pytest.raises(ValueError, match="depth"):
        api.png_encode_batch_lz(ok, depth=4)
    assert api.png_encode_batch_lz([]) == [] and api.png_encode_batch_lz(ok[:0]) == []
    sig, old = inspect.signature(api.png_encode_batch_lz), inspect.signature(api.png_encode_batch_dyn)
    assert list(sig.parameters) == list(old.parameters) == ["images", "layout", "depth", "palette", "trns", "filter", "level"]
    assert [p.default for p in sig.parameters.values()][1:] == ["hwc", None, None, None, "adaptive", 3]


# ---- the sanitizer program (stand-alone, a plain child process) --------------------------------------------------------------------

def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    import subprocess

    r = subprocess.run(["sh", os.path.join(ROOT, "tools", "asan_png_encode_lz_emu.sh"), str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
