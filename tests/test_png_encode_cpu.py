"""What of the PNG encode (include/decode_png.h: debig_png_encode_batch) can be checked without a device:
  * the numpy restatement tests/png_encode_ref.py against Pillow and against the pure-Python codec tests/png_spec_ref.py: for every
    colour type, both depths, a palette with and without tRNS, and every filter mode, a file assembled from the restated stream and
    zlib.compress decodes to the input; ADAPTIVE picks the expected type on rows made by hand;
  * the argument and descriptor rules of the C call that are decided before any device work: BAD_ARG, E_ENCODE rule by rule,
    debig_png_encode_bound; the ValueErrors of api.png_encode_batch."""
import ctypes as C
import inspect
import io
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_ref as R  # noqa: E402
import png_spec_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 0x10000  # "device pointers" that are never followed: every case below is decided before a device is touched


class Desc(C.Structure):  # include/decode_png.h: debig_png_encode_desc
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32), ("dtype", C.c_uint32), ("depth", C.c_uint32),
                ("layout", C.c_uint32), ("palette_entries", C.c_uint32), ("trns_entries", C.c_uint32), ("palette_off", C.c_uint64),
                ("trns_off", C.c_uint64)]


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
    L.debig_png_encode_bound.restype = C.c_uint64
    L.debig_png_encode_bound.argtypes = [C.POINTER(Desc)]
    L.debig_png_encode_batch.restype = C.c_int
    L.debig_png_encode_batch.argtypes = [C.c_void_p] * 7 + [C.c_uint32] * 3
    return L


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

def _image(seed, H, W, Cn, depth, top=None):
    rng = np.random.default_rng(seed)
    smooth = np.cumsum(rng.integers(-2, 3, (H, W, Cn)), axis=1) + (1 << (depth - 1))
    img = np.where(rng.integers(0, 3, (H, 1, 1)) == 0, rng.integers(0, 1 << depth, (H, W, Cn)), smooth)
    return np.clip(img, 0, (1 << depth) - 1 if top is None else top)


@pytest.mark.parametrize("filt", range(6))
@pytest.mark.parametrize("Cn,depth", [(1, 8), (2, 8), (3, 8), (4, 8), (1, 16), (2, 16), (3, 16), (4, 16)])
def test_a_file_from_the_restated_stream_decodes_to_the_input(Cn, depth, filt):
    Image = pytest.importorskip("PIL.Image")
    img = _image(Cn * 10 + filt, 13, 17, Cn, depth)
    stream = R.filtered_stream(img, depth, filt)
    assert len(stream) == 13 * (1 + 17 * Cn * depth // 8)
    if filt < 5:
        assert set(stream[:: 1 + 17 * Cn * depth // 8]) == {filt}
    data = R.container(17, 13, Cn, depth, zlib.compress(stream, 1))
    st, got, inf, _, _ = R.samples_of(data)
    assert st == S.OK and np.array_equal(got, img) and (inf["color_type"], inf["bit_depth"]) == (R.COLOR_TYPE[Cn], depth)
    st, rgba, _ = S.decode(data)
    assert st == S.OK
    pil = Image.open(io.BytesIO(data))
    pil.load()
    assert pil.size == (17, 13)
    if depth == 8:
        assert np.array_equal(np.asarray(pil).reshape(13, 17, Cn), img)
        assert np.array_equal(np.asarray(pil.convert("RGBA")), rgba)
    elif Cn == 1:
        assert np.array_equal(np.asarray(pil).astype(np.int64).reshape(13, 17, 1), img)  # (Pillow keeps 16 bits for grey only)


@pytest.mark.parametrize("trns", [None, 5, 21])
def test_a_palette_file_with_and_without_trns(trns):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    pal = rng.integers(0, 256, (21, 3), dtype=np.uint8)
    alpha = None if trns is None else rng.integers(0, 256, trns, dtype=np.uint8)
    img = np.repeat(np.repeat(rng.integers(0, 21, (5, 6, 1)), 3, axis=0), 4, axis=1)
    data = R.container(24, 15, 1, 8, zlib.compress(R.filtered_stream(img, 8, 5), 1), palette=pal, trns=alpha)
    st, got, inf, _, _ = R.samples_of(data)
    assert st == S.OK and np.array_equal(got, img) and inf["color_type"] == 3 and inf["has_trns"] == (trns is not None)
    st, rgba, _ = S.decode(data)
    want = np.concatenate([pal, np.full((21, 1), 255, np.uint8)], axis=1)
    if alpha is not None:
        want[: len(alpha), 3] = alpha
    assert st == S.OK and np.array_equal(rgba, want[img[:, :, 0]])
    pil = Image.open(io.BytesIO(data))
    assert pil.mode == "P" and np.array_equal(np.asarray(pil), img[:, :, 0]) and np.array_equal(np.asarray(pil.convert("RGBA")), rgba)
    assert len(data) <= R.bound(24, 15, 1, 8, 21, trns or 0)


def test_adaptive_on_rows_made_by_hand():
    ramp = np.arange(40, 80)
    rows = np.stack([np.zeros(40, np.int64),      # all zero: every type costs 0, the tie goes to 0
                     ramp,                        # a horizontal ramp under a zero row: Sub leaves 40, 1, 1, ...
                     ramp,                        # the row above again: Up leaves zeros
                     ramp[::-1] * 3 % 251])       # noise-like
    types = R.filter_types(R.raw_rows(rows[:, :, None], 8), 1, 5)
    assert types[:3].tolist() == [0, 1, 2]
    # a tie between two types goes to the lower one: in the first row Up equals None and Paeth equals Sub
    one = R.filter_types(R.raw_rows(np.array([[[3], [3], [3], [3]]]), 8), 1, 5)
    assert one.tolist() == [1]  # None / Up cost 12, Sub / Paeth 3, Average 3 + 2 + 2 + 2: Sub, not Paeth
    flat = R.filter_types(R.raw_rows(np.array([[[200], [200]]]), 8), 1, 5)
    assert flat.tolist() == [1] and R.filtered_stream(np.array([[[200], [200]]]), 8, 5) == bytes([1, 200, 0])
    # min(b, 256 - b): 255 counts as 1
    assert R.filter_types(R.raw_rows(np.array([[[255]]]), 8), 1, 5).tolist() == [0]
    assert R.filter_types(R.raw_rows(np.array([[[255], [254]]]), 8), 1, 5).tolist() == [1]  # None 1 + 2, Sub 1 + 1


def test_the_bound_and_the_chunk_cut():
    assert R.chunks(1) == [(0, 1)] and R.chunks(R.CHUNK) == [(0, R.CHUNK)] and R.chunks(R.CHUNK + 1) == [(0, R.CHUNK), (R.CHUNK, 1)]
    assert R.stored_payload(R.CHUNK + 1) == 5 + R.CHUNK + 5 + 5 + 1
    assert R.slot_bytes(R.CHUNK) % 16 == 0 and R.slot_bytes(R.CHUNK) >= (3 + 9 * R.CHUNK + 7 + 3 + 7) // 8 + 4
    assert R.row_runs(5, 70000) == [(y, 1) for y in range(5)] and R.row_runs(5, 30000) == [(0, 2), (2, 2), (4, 1)]


# ---- the C call --------------------------------------------------------------------------------------------------------------------

GOOD = dict(width=33, height=24, channels=3, dtype=0, depth=8, layout=0, palette_entries=0, trns_entries=0)
BAD_DESCS = [dict(width=0), dict(width=16385), dict(height=0), dict(height=16385), dict(channels=0), dict(channels=5),
             dict(channels=2, dtype=2, depth=16), dict(channels=3, dtype=3, depth=8), dict(dtype=4), dict(depth=16), dict(depth=4), dict(depth=0),
             dict(dtype=1, depth=8), dict(dtype=2, channels=1, depth=32), dict(layout=2), dict(palette_entries=4),
             dict(channels=1, palette_entries=257), dict(channels=1, dtype=1, depth=16, palette_entries=4),
             dict(channels=1, dtype=3, depth=16, palette_entries=4), dict(channels=1, palette_entries=4, trns_entries=5), dict(trns_entries=1)]
GOOD_DESCS = [dict(), dict(layout=1), dict(channels=1, dtype=2, depth=8), dict(channels=1, dtype=3, depth=16), dict(channels=4, dtype=1, depth=16),
              dict(channels=1, palette_entries=256, trns_entries=256), dict(channels=1, dtype=3, depth=8, palette_entries=1), dict(width=16384, height=1)]


def _call(lib, descs, ptrs, filt=5, level=1, side=b"\0" * 2048, outs=True, caps=None):
    n = len(descs)
    arr = (Desc * n)(*[Desc(**d) for d in descs])
    bufs = [(C.c_uint8 * 64)(*([0xAB] * 64)) for _ in range(n)]
    sizes, status = (C.c_uint64 * n)(*([77] * n)), (C.c_uint32 * n)(*([99] * n))
    rc = lib.debig_png_encode_batch((C.c_void_p * n)(*ptrs) if ptrs is not None else None, arr, side,
                                    (C.c_void_p * n)(*[C.addressof(b) for b in bufs]) if outs else None,
                                    (C.c_uint64 * n)(*(caps or [64] * n)), sizes, status, n, filt, level)
    assert all(bytes(b) == b"\xab" * 64 for b in bufs)
    return rc, list(status), list(sizes)


def test_c_argument_checks_come_before_any_device_work(lib):
    for kw in (dict(ptrs=None), dict(outs=False), dict(filt=6), dict(filt=2 ** 31), dict(level=2), dict(level=2 ** 32 - 1)):
        rc, status, sizes = _call(lib, [GOOD, GOOD], kw.pop("ptrs", [DUMMY, DUMMY]), **kw)
        assert rc == R.BAD_ARG and status == [99, 99] and sizes == [77, 77], kw
    n = 2
    arr = (Desc * n)(Desc(**GOOD), Desc(**GOOD))
    for hole in range(1, 7):  # descs, outs, out_caps, out_sizes, status NULL (side may be NULL without a palette)
        if hole == 2:
            continue
        args = [(C.c_void_p * n)(DUMMY, DUMMY), arr, None, (C.c_void_p * n)(), (C.c_uint64 * n)(), (C.c_uint64 * n)(), (C.c_uint32 * n)()]
        args[hole] = None
        assert lib.debig_png_encode_batch(*args, n, 5, 1) == R.BAD_ARG, hole
    rc, status, _ = _call(lib, [dict(GOOD, channels=1, palette_entries=4)], [DUMMY], side=None)
    assert rc == R.BAD_ARG and status == [99]
    # n == 0 is fine and touches nothing, whatever else is passed
    assert lib.debig_png_encode_batch(None, None, None, None, None, None, None, 0, 9, 9) == 0


def test_every_descriptor_rule_gives_e_encode_and_a_bound_of_zero(lib):
    descs = [dict(GOOD, **b) for b in BAD_DESCS]
    for d in descs:
        assert lib.debig_png_encode_bound(C.byref(Desc(**d))) == 0, d
    rc, status, sizes = _call(lib, descs, [DUMMY] * len(descs))  # a batch of bad descriptors only: no device work at all
    assert rc == 0 and status == [R.E_ENCODE] * len(descs) and sizes == [0] * len(descs)
    # an image pointer that is NULL or not aligned to its element
    ptr_cases = [(dict(GOOD), None), (dict(GOOD, channels=1, dtype=1, depth=16), DUMMY + 1), (dict(GOOD, channels=1, dtype=2, depth=8), DUMMY + 2),
                 (dict(GOOD, channels=1, dtype=3, depth=16), DUMMY + 4)]
    rc, status, _ = _call(lib, [d for d, _ in ptr_cases], [p for _, p in ptr_cases])
    assert rc == 0 and status == [R.E_ENCODE] * 4
    assert lib.debig_png_encode_bound(None) == 0


def test_the_bound_is_the_level_0_file(lib):
    for g in GOOD_DESCS + [dict(width=300, height=300), dict(width=1024, height=1024, channels=4, dtype=1, depth=16)]:
        d = dict(GOOD, **g)
        assert lib.debig_png_encode_bound(C.byref(Desc(**d))) == R.bound(d["width"], d["height"], d["channels"], d["depth"], d["palette_entries"],
                                                                        d["trns_entries"]), d


def test_symbols_constants_and_documents(lib, api):
    for name in ("debig_png_encode_batch", "debig_png_encode_bound", "debig_hip_png_encode_filter_batch", "debig_hip_png_encode_deflate_batch"):
        assert hasattr(lib, name), name
    pub = open(os.path.join(ROOT, "include", "decode_png.h")).read()
    dev = open(os.path.join(ROOT, "include", "debig_hip.h")).read()
    for text in ("#define DEBIG_PNG_E_ENCODE 20", "#define DEBIG_PNG_E_RANGE 21", "DEBIG_PNG_FILTER_ADAPTIVE = 5", "int debig_png_encode_batch(",
                 "SYNCHRONOUS", "NOT THREAD SAFE", "dynamic Huffman blocks, lazy matching, levels above 1", "Adam7", "host tensors"):
        assert text in pub, text
    for text in ("#define DEBIG_PNG_ENCODE_CHUNK %du" % R.CHUNK, "#define DEBIG_PNG_ENCODE_FILTER_BYTES %du" % R.FILTER_BYTES,
                 "_png_encode_filter / _png_encode_deflate", "} debig_png_encode_deflate_task;", "#define DEBIG_PNG_ENCODE_NO_STORED 1u"):
        assert text in dev, text
    assert 8192 <= R.CHUNK <= 65536
    assert api.PNG_STATUS[R.E_ENCODE] == "encode" and api.PNG_STATUS[R.E_RANGE] == "range" and api.PNG_STATUS[R.E_OUTPUT] == "output"
    assert api.PNG_ENCODE_FILTERS == R.FILTERS


# ---- Python ------------------------------------------------------------------------------------------------------------------------

def test_png_encode_batch_argument_rules(api):
    import torch

    ok = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        api.png_encode_batch(ok)
    with pytest.raises(ValueError, match="GPU"):
        api.png_encode_batch([ok[0], ok[1, :, :, 0]])
    for f in ("best", 5, None, "ADAPTIVE"):
        with pytest.raises(ValueError, match="filter"):
            api.png_encode_batch(ok, filter=f)
    for lv in (2, -1, "1", None, True, 9):
        with pytest.raises(ValueError, match="level"):
            api.png_encode_batch(ok, level=lv)
    for d in (4, 32, "8", True):
        with pytest.raises(ValueError, match="depth"):
            api.png_encode_batch(ok, depth=d)
    with pytest.raises(ValueError, match="layout"):
        api.png_encode_batch(ok, layout="nhwc")
    for dt in (torch.float32, torch.int8, torch.bool, torch.float16):
        with pytest.raises(ValueError, match="uint8, uint16"):
            api.png_encode_batch(torch.zeros((2, 4, 5), dtype=dt))
    for t in (torch.zeros((4, 5), dtype=torch.uint8), torch.zeros((1, 2, 4, 5, 3), dtype=torch.uint8), np.zeros((2, 4, 5), np.uint8), None):
        with pytest.raises(ValueError, match="tensor"):
            api.png_encode_batch(t)
    for t in ([torch.zeros((5,), dtype=torch.uint8)], [torch.zeros((1, 2, 4, 5), dtype=torch.uint8)], [np.zeros((4, 5), np.uint8)]):
        with pytest.raises(ValueError, match="an image must be"):
            api.png_encode_batch(t)
    grey = torch.zeros((2, 4, 5), dtype=torch.uint8)
    for pal in (np.zeros((4, 4), np.uint8), np.zeros((0, 3), np.uint8), np.zeros((257, 3), np.uint8), np.zeros((4, 3), np.int32), np.zeros(12, np.uint8)):
        with pytest.raises(ValueError, match="palette must"):
            api.png_encode_batch(grey, palette=pal)
    with pytest.raises(ValueError, match="one entry per image"):
        api.png_encode_batch(grey, palette=[np.zeros((4, 3), np.uint8)])
    with pytest.raises(ValueError, match="trns must"):
        api.png_encode_batch(grey, palette=np.zeros((4, 3), np.uint8), trns=np.zeros((4, 1), np.uint8))
    assert api.png_encode_batch([]) == [] and api.png_encode_batch(grey[:0]) == []
    sig = inspect.signature(api.png_encode_batch)
    assert list(sig.parameters) == ["images", "layout", "depth", "palette", "trns", "filter", "level"]
    assert [p.default for p in sig.parameters.values()][1:] == ["hwc", None, None, None, "adaptive", 1]


# ---- the sanitizer program (stand-alone, a plain child process) --------------------------------------------------------------------

def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    import subprocess

    r = subprocess.run(["sh", os.path.join(ROOT, "tools", "asan_png_encode_emu.sh"), str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all checks passed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
