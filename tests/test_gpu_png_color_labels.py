"""debig_png_decode_batch_color_labels on the MI355X (include/decode_png.h; api.png_decode_batch_color_labels): the whole call
BIT FOR BIT against the numpy restatement (tests/png_color_label_ref.py) -- every colour type, depth, interlace and tRNS
combination and RGB / RGBA / palette mask files of other sizes in ONE batch, PACK to both dtypes, MAP to all four with a shared
map that covers part of the colours, `unmatched` exact; per-image maps; against the calls that already exist; per-image boxes;
E_LABEL / E_BOX and their order; bad files in the middle of a batch with a sentinel-filled tensor; every BAD_ARG rule; nothing
outside the tensor written; the raw-label call still refuses an RGB file."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_label_ref as CR  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_gpu_png_spec as G  # noqa: E402
import test_png_color_labels_cpu as CPU  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ["uint8", "uint16", "int32", "int64"]
RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resources")


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


def _colour_list(rng, n):
    ks = {0x000000, 0xFFFFFF}
    while len(ks) < n:
        ks.add(int(rng.integers(0, 1 << 24)))
    ks = np.array(sorted(ks), dtype=np.uint32)
    return np.stack([ks & 255, (ks >> 8) & 255, ks >> 16], axis=-1).astype(np.uint8)


def _mask_file(rng, w, h, colours, kind, il=0):
    """a blocky mask of w x h drawn from `colours` ((m, 3) uint8), stored as RGB, RGBA or (m <= 256) palette"""
    idx = np.kron(rng.integers(0, len(colours), size=((h + 3) // 4, (w + 4) // 5)), np.ones((4, 5), dtype=np.int64))[:h, :w]
    if kind == "pal":
        return R.encode(idx[:, :, None].astype(np.uint8), 3, 8, il, palette=[tuple(int(v) for v in c) for c in colours],
                        filters=lambda p, y: y % 5)
    px = colours[idx]
    if kind == "rgba":
        px = np.concatenate([px, rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8)], axis=2)
    return R.encode(px, 6 if kind == "rgba" else 2, 8, il, filters=lambda p, y: y % 5)


_D = {}


def _data():
    """every file of _all_formats() (45 x 70: every colour type, depth, interlace, tRNS) with RGB / RGBA / palette masks of
    1 x 1, 64 x 65, 333 x 129 and 5 x 300 from 7, 200 and 2048 colours interleaved; the shared map covers part of the colours"""
    if not _D:
        rng = np.random.default_rng(79)
        c7, c200, c2048 = _colour_list(rng, 7), _colour_list(rng, 200), _colour_list(rng, 2048)
        masks = [_mask_file(rng, 1, 1, c7, "rgb"), _mask_file(rng, 64, 65, c7, "pal"), _mask_file(rng, 333, 129, c200, "rgba", 1),
                 _mask_file(rng, 5, 300, c200, "pal"), _mask_file(rng, 64, 65, c2048, "rgb", 1), _mask_file(rng, 333, 129, c2048, "rgb"),
                 _mask_file(rng, 5, 300, c7, "rgba"), _mask_file(rng, 64, 65, c200, "rgb")]
        out = []
        for k, f in enumerate(d for _, d in G._all_formats()):
            out.append(f)
            if k % 5 == 0 and masks:
                out.append(masks.pop())
        _D["files"] = out + masks
        keys = np.concatenate([CR.pack(c7)[:5], CR.pack(c200)[::2], CR.pack(c2048)[::3], [0x555555, 0xAAAAAA, 0x111111]])
        _D["keys"] = [int(k) for k in dict.fromkeys(int(k) for k in keys)]
        _D["c7"], _D["c200"] = c7, c200
    return _D


@pytest.fixture(scope="module")
def datas():
    return _data()["files"]


_REF = {}


def _ref(data):
    """the restatement's RGB8 pixels of a file, computed once"""
    if data not in _REF:
        _REF[data] = CR.rgb(data)
    return _REF[data]


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _values(keys, dtype, seed=0):
    top = {"uint8": 255, "uint16": 65535}.get(dtype)  # (the top value is kept for `missing`)
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, top, len(keys)) if top else rng.integers(-2 ** 31, 2 ** 31, len(keys))
    return {int(k): int(v) for k, v in zip(keys, vals)}


def _as_colors(m):
    """a restatement map {key: value} -> the (keys, values) pair of the Python call"""
    return np.array(list(m.keys()), dtype=np.uint32), np.array(list(m.values()), dtype=np.int64)


def _check(api, datas, size, dtype, maps=None, missing=-1, boxes=None, fill=None, expect=None):
    """maps: None (PACK), one dict {key: value}, or a list of one dict per file"""
    colors = None if maps is None else [_as_colors(m) for m in maps] if isinstance(maps, list) else _as_colors(maps)
    st, t, infos, um = api.png_decode_batch_color_labels(datas, size, colors, missing, dtype, boxes=boxes, fill=fill)
    got = _np(t)
    assert got.shape == (len(datas),) + tuple(size) and got.dtype == CR.DTYPES[dtype]
    for i, data in enumerate(datas):
        rst, px, inf = _ref(data)
        box = boxes[i] if boxes is not None else None
        want = rst
        if inf["width"] and inf["bit_depth"] == 16:
            want = CR.E_LABEL
        elif inf["width"] and CR.LR.box_error(box, inf["width"], inf["height"]):
            want = CR.E_BOX
        if expect is not None:
            assert want == expect[i], (i, want, expect[i])
        assert st[i] == want, (i, inf, st[i], want)
        if rst == 0:
            assert infos[i] == inf, i
        if st[i] != 0:
            assert um[i] == 0, i
            if fill is not None:
                assert (got[i] == np.array(fill).astype(got.dtype)).all(), (i, "a failed file's slot was written")
            continue
        m = maps[i] if isinstance(maps, list) else maps
        exp, miss = CR.gather(px, size, box, m, missing, dtype)
        assert got[i].tobytes() == exp.tobytes(), (i, inf, size, dtype, box, np.argwhere(got[i] != exp)[:4])
        assert um[i] == miss, (i, um[i], miss)
    return st, um


def _label_statuses(datas, st):
    for data, s in zip(datas, st):
        assert s == (CR.E_LABEL if _ref(data)[2]["bit_depth"] == 16 else 0)


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_mixed_batch_packed(api, datas, dtype):
    for size in ((32, 24), (75, 50)):
        st, um = _check(api, datas, size, dtype)
        _label_statuses(datas, st)
        assert um == [0] * len(datas)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_batch_with_a_shared_map(api, datas, dtype):
    """the map covers 5 of the 7, every second of the 200 and every third of the 2048 colours: every mask has misses"""
    m = _values(_data()["keys"], dtype, 5)
    missing = {"uint8": 255, "uint16": 65535}.get(dtype, -1)
    for size in ((32, 24), (75, 50)):
        st, um = _check(api, datas, size, dtype, m, missing)
        _label_statuses(datas, st)
        assert sum(1 for u in um if u) > 8 and any(u == size[0] * size[1] for u in um)


def test_per_image_maps_like_coco_panoptic(api):
    """few segments per image, the colour IS the segment id, a different id -> category table per image; one image whose
    table is empty, one whose table lacks a segment"""
    rng = np.random.default_rng(11)
    files, maps = [], []
    for k, (w, h) in enumerate([(64, 65), (333, 129), (5, 300), (1, 1), (64, 65), (45, 70)]):
        ids = rng.choice(1 << 24, size=3 + 2 * k, replace=False).astype(np.uint32)
        colours = np.stack([ids & 255, (ids >> 8) & 255, ids >> 16], axis=-1).astype(np.uint8)
        files.append(_mask_file(rng, w, h, colours, ("rgb", "rgba", "pal")[k % 3], k % 2))
        maps.append({int(i): int(c) for i, c in zip(ids, rng.integers(1, 134, len(ids)))})
    maps[4] = {}
    del maps[5][next(iter(maps[5]))]
    for dtype, size in (("int64", (75, 50)), ("uint8", (32, 24))):
        st, um = _check(api, files, size, dtype, maps, 0)
        assert st == [0] * 6 and um[4] == size[0] * size[1] and um[:3] == [0, 0, 0]
    # the packed call gives the segment ids themselves
    st, t, _, _ = api.png_decode_batch_color_labels(files, (75, 50), dtype="int64")
    assert st == [0] * 6
    for i in range(4):
        assert set(int(v) for v in np.unique(_np(t)[i])) <= set(maps[i])


def test_against_the_calls_that_exist(api, datas):
    good = [d for d in datas if _ref(d)[0] == 0]
    # PACK at the file's own size: png_decode_batch(mode="rgb") packed
    for data, (hst, px, inf) in zip(good[::4], api.png_decode_batch(good[::4], mode="rgb")):
        st, t, _, _ = api.png_decode_batch_color_labels([data], (inf["height"], inf["width"]), dtype="int32")
        assert st == [0] and hst == 0 and np.array_equal(_np(t)[0], CR.pack(px).astype(np.int32))
    # PACK resized: the nearest filter of the tensor call, packed, with the same boxes
    boxes = []
    for i, data in enumerate(good):
        inf = _ref(data)[2]
        w, h = inf["width"], inf["height"]
        boxes.append([None, (0, 0, max(w // 2, 1), max(h // 3, 1)), (w - 1, 0, 1, h), (w - max(w // 3, 1), h - max(h // 2, 1), max(w // 3, 1), max(h // 2, 1))][i % 4])
    for size in ((32, 24), (75, 50)):
        for bx in (None, boxes):
            st, t, _, _ = api.png_decode_batch_color_labels(good, size, dtype="int64", boxes=bx)
            st2, t2, _ = api.png_decode_batch_tensor(good, size, mode="rgb", depth=8, dtype="uint", layout="hwc", boxes=bx, filter="nearest")
            assert st == st2 == [0] * len(good)
            assert np.array_equal(_np(t), CR.pack(_np(t2)).astype(np.int64)), size


def _palette_agreement(api, data, size):
    """the map {PLTE[i]: i} (first occurrence of a colour wins): the labels' colours are those of the raw-label call's
    indices run through PLTE"""
    pal = R._walk(data)[2][0][:, :3]
    keys = CR.pack(pal)
    m = {}
    for i, k in enumerate(keys):
        m.setdefault(int(k), i)
    st, t, _, um = api.png_decode_batch_color_labels([data], size, _as_colors(m), -1, "int64")
    st2, t2, _ = api.png_decode_batch_labels([data], size, dtype="int64")
    assert st == st2 == [0] and um == [0]
    a, b = _np(t)[0], _np(t2)[0]
    assert a.min() >= 0 and np.array_equal(keys[a], keys[b])
    return a


def test_palette_files_agree_with_the_raw_label_call(api, datas):
    rng = np.random.default_rng(21)
    dup = np.concatenate([_data()["c7"], _data()["c7"][:3], _data()["c200"][:50]])  # colours that occur twice in PLTE
    for data in [_mask_file(rng, 64, 65, dup, "pal"), _mask_file(rng, 333, 129, _data()["c200"], "pal", 1)]:
        for size in ((65, 64), (32, 24)):
            _palette_agreement(api, data, size)
    # the first colour-type-3 file of tests/golden/resources
    paths = sorted(glob.glob(os.path.join(RES, "*.png")))
    data = next(d for d in (open(p, "rb").read() for p in paths) if api.png_info(d)[1]["color_type"] == 3)
    inf = api.png_info(data)[1]
    a = _palette_agreement(api, data, (inf["height"], inf["width"]))
    hst, rgb, _ = api.png_decode_batch([data], mode="rgb")[0]
    pal = R._walk(data)[2][0][:, :3]
    assert hst == 0 and np.array_equal(pal[a], rgb)
    _palette_agreement(api, data, (48, 40))


def test_per_image_boxes_and_the_order_of_label_and_box_errors(api, datas):
    boxes = []
    for i, data in enumerate(datas):
        _, inf = api.png_info(data)
        w, h = inf["width"], inf["height"]
        boxes.append([None, (0, 0, 0, 0), (0, 0, max(w // 2, 1), max(h // 3, 1)), (w - max(w // 3, 1), h - max(h // 2, 1), max(w // 3, 1), max(h // 2, 1)),
                      (w - 1, 0, 1, h), (0, h - 1, w, 1)][i % 6])
    _check(api, datas, (20, 16), "int64", _values(_data()["keys"], "int64", 1), -1, boxes=boxes)
    _check(api, datas, (20, 16), "int32", boxes=boxes)
    _check(api, datas, (20, 16), "uint8", _values(_data()["keys"], "uint8", 2), 255, boxes=boxes)
    rng = np.random.default_rng(3)
    rgb = R.encode(R.random_image(rng, 45, 70, 2, 8), 2, 8, 1)
    rgb16 = R.encode(R.random_image(rng, 45, 70, 2, 16), 2, 16)
    g4 = R.encode(R.random_image(rng, 45, 70, 0, 4), 0, 4, 1)
    files = [rgb, rgb, g4, g4, rgb16, rgb16, rgb[:60], rgb]
    bxs = [None, (40, 0, 6, 5), (0, 0, 0, 9), (5, 6, 7, 8), (0, 0, 46, 1), None, (0, 0, 46, 1), (0, 69, 45, 1)]
    B, Lb = CR.E_BOX, CR.E_LABEL
    st, _ = _check(api, files, (3, 9), "int32", boxes=bxs, fill=-9, expect=[0, B, B, 0, Lb, Lb, B, 0])
    assert st == [0, B, B, 0, Lb, Lb, B, 0]


def test_bad_files_in_the_middle_of_a_batch_leave_their_slots(api, datas):
    """the damaged files of test_gpu_png_spec._error_files(), b"not a png" and a truncated file between good ones: the statuses
    of png_decode_batch, except E_LABEL on 16-bit files; slots untouched, unmatched 0"""
    cases = G._error_files()
    good = [d for d in datas if _ref(d)[0] == 0][:4]
    batch = good[:2] + [d for _, d, _ in cases] + [b"not a png", good[3][:40]] + good[2:]
    plain = [s for s, _, _ in api.png_decode_batch(batch)]
    m = _values(_data()["keys"], "uint16", 8)
    for dtype, fill, maps, missing in (("int64", -77, None, -1), ("uint8", 0xA5, {k: v & 127 for k, v in m.items()}, 200), ("uint16", 0xBEEF, m, 65535)):
        st, um = _check(api, batch, (19, 21), dtype, maps, missing, fill=fill)
        for k, (data, s, p) in enumerate(zip(batch, st, plain)):
            inf = _ref(data)[2]
            assert s == (CR.E_LABEL if inf["width"] and inf["bit_depth"] == 16 else p), (k, s, p)
        assert st[:2] == [0, 0] and st[-2:] == [0, 0] and st[-4:-2] == [R.E_SIGNATURE, R.E_CHUNK]


def _c_call(api):
    L = api._png_spec_lib()
    L.debig_png_decode_batch_color_labels.restype = C.c_int
    L.debig_png_decode_batch_color_labels.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p]
    return L.debig_png_decode_batch_color_labels


def test_every_bad_arg_rule_leaves_status_unmatched_and_tensor(api, datas):
    import torch

    call = _c_call(api)
    files = [d for d in datas if _ref(d)[0] == 0][:3]
    n = len(files)
    ins = [np.frombuffer(f, np.uint8) for f in files]
    arena = torch.full((n * 6 * 8 * 8 + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for name, desc, off in CPU.bad_arg_cases(n):
        st = (C.c_uint32 * n)(*[0xABCD] * n)
        um = (C.c_uint32 * n)(*[0xABCD] * n)
        rc = call((C.c_void_p * n)(*[a.ctypes.data for a in ins]), (C.c_uint64 * n)(*[len(f) for f in files]),
                  None if off is None else arena.data_ptr() + off, None, st, None, um, n, 0, C.byref(desc) if desc is not None else None)
        assert rc == api.PNG_BAD_ARG and list(st) == [0xABCD] * n and list(um) == [0xABCD] * n, name
    torch.cuda.synchronize()
    assert (arena.cpu().numpy() == 0xA5).all()
    # the Python call turns the C call's refusal into ValueError
    for kw in (dict(colors=(np.array([5, 5]), np.array([1, 2]))), dict(colors=(np.array([1 << 24]), np.array([1]))),
               dict(colors=(np.arange(2049), np.arange(2049))), dict(colors={(1, 2, 3): 300}, dtype="uint8", missing=0),
               dict(colors={(1, 2, 3): 3}, dtype="uint8", missing=-1)):
        with pytest.raises(ValueError):
            api.png_decode_batch_color_labels(files, (6, 8), **kw)


def test_nothing_outside_the_tensor_is_written(api, datas):
    """the C call on a slice in the middle of a sentinel-filled allocation"""
    import torch
    from debigulator_amd import _native as N

    call = _c_call(api)
    ok = [d for d in datas if _ref(d)[0] == 0]
    files = ok[:5] + [b"not a png"] + ok[5:10]
    n = len(files)
    ins = [np.frombuffer(f, np.uint8) for f in files]
    m = _values(_data()["keys"], "uint8", 4)
    for dtype, size, maps in (("int64", (13, 100), None), ("uint8", (33, 31), m), ("int64", (33, 31), m), ("uint8", (13, 100), m)):
        d, es = api.png_color_label_desc(size, None if maps is None else _as_colors(maps), 255, dtype, n)
        slot = size[0] * size[1] * es
        arena = torch.full((4096 + n * slot + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        st = (C.c_uint32 * n)()
        um = (C.c_uint32 * n)(*[7] * n)
        rc = call((C.c_void_p * n)(*[a.ctypes.data for a in ins]), (C.c_uint64 * n)(*[len(f) for f in files]),
                  arena.data_ptr() + 4096, None, st, None, um, n, 0, C.byref(d))
        N.check(rc, "debig_png_decode_batch_color_labels")
        a = arena.cpu().numpy()
        assert list(st) == [0] * 5 + [R.E_SIGNATURE] + [0] * 5 and um[5] == 0
        assert (a[:4096] == 0xA5).all() and (a[4096 + n * slot:] == 0xA5).all() and (a[4096 + 5 * slot: 4096 + 6 * slot] == 0xA5).all()
        for i in (0, 4, 6, 10):
            want, miss = CR.gather(_ref(files[i])[1], size, None, maps, 255, dtype)
            assert a[4096 + i * slot: 4096 + (i + 1) * slot].tobytes() == want.tobytes(), (dtype, size, i)
            assert um[i] == miss


def test_the_raw_label_call_still_refuses_an_rgb_file(api):
    rng = np.random.default_rng(1)
    rgb = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    st, _, _ = api.png_decode_batch_labels([rgb], (7, 9))
    assert st == [CR.E_LABEL]
