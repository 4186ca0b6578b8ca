"""debig_png_decode_batch_tensor_filter on the MI355X (include/decode_png.h; api.png_decode_batch_tensor(filter=...)): the whole
call with filter "bicubic" and "nearest", BIT FOR BIT against the numpy restatement (tests/png_filter_ref.py) applied to the
pixels of the existing host call api.png_decode_batch -- every colour type and depth, Adam7, tRNS and tuned-route files at
mixed sizes in ONE batch and real files of tests/golden/resources; straight, OVER and PREMULTIPLIED; every dtype, both
layouts; per-image boxes; the E_BOX scale of each filter; bad files in the middle of a batch with a sentinel-filled tensor;
nothing outside the tensor written; filter="bilinear" against the call without the argument."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_alpha_ref as A  # noqa: E402
import png_filter_ref as F  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_gpu_png_spec as G  # noqa: E402

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
CH = {"rgba": 4, "rgb": 3, "gray": 1, "gray_alpha": 2}
WITH_ALPHA = {"rgb": "rgba", "gray": "gray_alpha", "rgba": "rgba", "gray_alpha": "gray_alpha"}
DTYPES = ["uint", "float32", "float16", "bfloat16"]
BACKGROUNDS = [None, 0.0, (0.25, 1.0, 0.6)]
FILTERS = ["bicubic", "nearest"]
RES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resources")


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


@pytest.fixture(scope="module")
def datas():
    """every colour type / depth / Adam7 / tRNS combination (45 x 70) and tuned-route files (8-bit RGB / RGBA, not
    interlaced) of other sizes, interleaved -- the batch of test_gpu_png_tensor.py"""
    rng = np.random.default_rng(77)
    fs = [d for _, d in G._all_formats()]
    tuned = [R.encode(R.random_image(rng, w, h, ct, 8), ct, 8, filters=lambda p, y: y % 5)
             for ct in (2, 6) for w, h in ((1, 1), (64, 65), (333, 129), (5, 300))]
    out = []
    for k, f in enumerate(fs):
        out.append(f)
        if k % 5 == 0 and tuned:
            out.append(tuned.pop())
    return out + tuned


@pytest.fixture(scope="module")
def real():
    """real files: RGB, palette, RGBA; 10 x 10 up to 1204 x 312"""
    return [open(os.path.join(RES, n), "rb").read() for n in ("backgrounddetailed1.png", "extraturns.png", "font.png",
                                                               "structuredart1.png", "purpleback.png")]


def _np(t):
    """a result tensor on the host: 16-bit integers as uint16, bfloat16 as its bit patterns (uint16)"""
    import torch

    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


_HOST = {}


def _host(api, data, mode, depth):
    if (data, mode, depth) not in _HOST:
        _HOST[(data, mode, depth)] = api.png_decode_batch([data], mode=mode, depth=depth)[0]
    return _HOST[(data, mode, depth)]


def _check(api, datas, size, filt, alpha, mode, depth=8, combos=(("float32", "chw"),), aa=True, boxes=None, background=None,
           fill=None, expect=None):
    """one integer reference per file, converted for every (dtype, layout) of combos; one device call per combo"""
    ch = CH[mode]
    src_mode = mode if alpha == "straight" else WITH_ALPHA[mode]
    akw, bgs = {}, None
    if alpha == "over":
        if background is not None and hasattr(background, "__len__"):
            background = background[:ch]
        bgs = A.background_samples(background, ch, depth)
        akw = dict(background=background)
    ref = {}
    st = None
    for dtype, layout in combos:
        kw = dict(mean=MEAN[:ch], std=STD[:ch]) if dtype != "uint" else {}
        st, t, infos = api.png_decode_batch_tensor(datas, size, mode=mode, depth=depth, dtype=dtype, layout=layout, boxes=boxes,
                                                   antialias=aa, fill=fill, alpha=alpha, filter=filt, **akw, **kw)
        d = api.png_tensor_desc(size, mode, depth, dtype, layout, antialias=aa, **kw)[0]
        got = _np(t)
        assert got.shape == ((len(datas), ch) + tuple(size) if layout == "chw" else (len(datas),) + tuple(size) + (ch,))
        for i, data in enumerate(datas):
            hst, px, hinf = _host(api, data, src_mode, depth)
            box = boxes[i] if boxes is not None else None
            want_st = expect[i] if expect is not None else hst
            assert st[i] == want_st, (i, st[i], want_st)
            if hst == 0:
                assert infos[i] == hinf, i
            if st[i] != 0:
                if fill is not None:
                    sentinel = Z.bf16_bits(np.float32(fill)) if dtype == "bfloat16" else np.array(fill).astype(got.dtype)
                    assert (got[i] == sentinel).all(), (i, "a failed file's slot was written")
                continue
            if i not in ref:
                ref[i] = (F.resize_int(px, size, filt, aa, box) if alpha == "straight" else
                          F.resize_alpha_int(px, size, filt, alpha, aa, box, bgs))
            v, P = ref[i]
            want = Z.convert(v, P, dtype, list(d.scale), list(d.bias))
            if layout == "chw":
                want = np.ascontiguousarray(np.transpose(want, (2, 0, 1)))
            assert got[i].dtype == want.dtype and got[i].shape == want.shape, (i, got[i].dtype, want.dtype)
            assert got[i].tobytes() == want.tobytes(), (i, hinf, size, filt, alpha, mode, depth, dtype, layout, aa, box, bgs,
                                                        np.argwhere(got[i] != want)[:4])
    return st


ALL_COMBOS = [(dt, lay) for dt in DTYPES for lay in ("chw", "hwc")]
MODES = [("straight", "rgb", 8), ("straight", "rgba", 16), ("straight", "gray", 16), ("straight", "gray_alpha", 8),
         ("over", "rgb", 8), ("over", "rgb", 16), ("over", "gray", 8), ("over", "gray", 16),
         ("premultiplied", "rgba", 8), ("premultiplied", "rgba", 16), ("premultiplied", "gray_alpha", 8),
         ("premultiplied", "gray_alpha", 16)]


@pytest.mark.parametrize("alpha,mode,depth", MODES)
@pytest.mark.parametrize("filt", FILTERS)
def test_mixed_batch_every_mode_format_dtype_and_layout(api, datas, filt, alpha, mode, depth):
    """1, 2, 3 and 4 channels, P = 8 and 16, every colour type, Adam7 and tRNS in one batch: shrinking with antialias for every
    dtype and layout, enlarging without for two of them"""
    k = MODES.index((alpha, mode, depth))
    st = _check(api, datas, (32, 24), filt, alpha, mode, depth, ALL_COMBOS, aa=True, background=BACKGROUNDS[k % 3])
    assert st == [0] * len(datas)
    _check(api, datas, (75, 50), filt, alpha, mode, depth, [ALL_COMBOS[k % 8], ALL_COMBOS[(k + 3) % 8]], aa=False,
           background=BACKGROUNDS[(k + 1) % 3])


@pytest.mark.parametrize("filt", FILTERS)
def test_real_files_to_224_chw_float32_and_other_shapes(api, real, datas, filt):
    st = _check(api, real + datas[:4], (224, 224), filt, "straight", "rgb")
    assert st == [0] * (len(real) + 4)
    _check(api, real, (48, 40), filt, "over", "rgb", combos=[("bfloat16", "hwc"), ("uint", "chw")], background=(0.0, 0.5, 1.0))
    _check(api, real[2:], (100, 61), filt, "premultiplied", "rgba", depth=16, combos=[("float16", "chw")], aa=False)
    _check(api, real[:4], (400, 400), filt, "straight", "gray", combos=[("uint", "hwc")])  # shrunk, unscaled, enlarged a little and enlarged 40 x


@pytest.mark.parametrize("filt", FILTERS)
def test_per_image_boxes(api, datas, filt):
    boxes = []
    for i, data in enumerate(datas):
        _, inf = api.png_info(data)
        w, h = inf["width"], inf["height"]
        k = i % 6
        boxes.append([None, (0, 0, 0, 0), (0, 0, max(w // 2, 1), max(h // 3, 1)), (w - max(w // 3, 1), h - max(h // 2, 1), max(w // 3, 1), max(h // 2, 1)),
                      (w - 1, 0, 1, h), (0, h - 1, w, 1)][k])
    for aa in (True, False):
        st = _check(api, datas, (20, 16), filt, "over", "rgb", 8, [("float32", "chw")], aa=aa, boxes=boxes, background=(1.0, 0.0, 0.5))
        assert st == [0] * len(datas)
        _check(api, datas, (20, 16), filt, "straight", "rgb", 16, [("uint", "hwc")], aa=aa, boxes=boxes)
        _check(api, datas, (20, 16), filt, "premultiplied", "gray_alpha", 8, [("float16", "hwc")], aa=aa, boxes=boxes)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("alpha,mode", [("straight", "rgb"), ("over", "rgb"), ("premultiplied", "rgba")])
def test_bad_files_in_the_middle_of_a_batch_leave_their_slots(api, datas, filt, alpha, mode):
    cases = G._error_files()
    good = datas[:4]
    batch = good[:2] + [d for _, d, _ in cases] + [b"not a png", datas[7][:40]] + good[2:]
    fmt_status = [s for s, _, _ in api.png_decode_batch(batch, mode="rgb", depth=8)]
    assert fmt_status[2: 2 + len(cases)] == [s for _, _, s in cases] and fmt_status[:2] == [0, 0] and fmt_status[-2:] == [0, 0]
    for dtype, fill, layout in (("float32", -7.5, "chw"), ("uint", 0xA5, "hwc"), ("bfloat16", 3.0, "hwc")):
        st = _check(api, batch, (19, 21), filt, alpha, mode, 8, [(dtype, layout)], fill=fill, background=(0.1, 0.9, 0.4) if alpha == "over" else None)
        assert st == fmt_status  # statuses as every tensor call gives them; the failed slots hold the fill


def test_box_errors_and_the_scale_rule_of_each_filter(api, datas):
    rng = np.random.default_rng(3)
    tall = R.encode(R.random_image(rng, 3, 100, 4, 8), 4, 8)   # 100 rows to 3: above 32, below 64
    taller = R.encode(R.random_image(rng, 3, 200, 4, 8), 4, 8)  # 200 rows to 3: above 64
    files = [datas[0], datas[1], tall, taller, datas[2], datas[3], datas[4][:60], datas[5]]
    boxes = [None, (40, 0, 6, 5), None, None, (0, 0, 0, 9), (5, 6, 7, 8), (0, 0, 46, 1), (0, 69, 45, 1)]
    B = Z.E_BOX
    for filt, aa, expect in (("bicubic", True, [0, B, B, B, B, 0, B, 0]), ("bicubic", False, [0, B, 0, 0, B, 0, B, 0]),
                             ("nearest", True, [0, B, 0, 0, B, 0, B, 0]), ("nearest", False, [0, B, 0, 0, B, 0, B, 0]),
                             ("bilinear", True, [0, B, 0, B, B, 0, B, 0])):
        st = _check(api, files, (3, 9), filt, "over", "rgb", 8, [("float32", "chw")], aa=aa, boxes=boxes, fill=9.0, expect=expect)
        assert st == expect, (filt, aa)
    # exactly 32 x: 96 rows to 3 pass, 97 do not
    edge = [R.encode(R.random_image(rng, 3, h, 2, 8), 2, 8) for h in (96, 97)]
    assert _check(api, edge, (3, 9), "bicubic", "straight", "rgb", 8, [("uint", "hwc")], fill=7, expect=[0, B]) == [0, B]


def test_nothing_outside_the_tensor_is_written(api, datas, real):
    """the C call on a slice in the middle of a sentinel-filled allocation"""
    import torch
    from debigulator_amd import _native as N

    L = api._png_spec_lib()
    L.debig_png_decode_batch_tensor_filter.restype = C.c_int
    L.debig_png_decode_batch_tensor_filter.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    files = datas[:5] + [b"not a png"] + datas[5:9] + real[2:3]
    n = len(files)
    for filt, alpha, mode, size in (("bicubic", "over", "rgb", (33, 31)), ("bicubic", "straight", "gray_alpha", (70, 45)),
                                    ("nearest", "premultiplied", "rgba", (13, 100)), ("bicubic", "straight", "rgb", (13, 200))):
        d, ch, es = api.png_tensor_desc(size, mode, 8, "float32", "hwc", MEAN[:CH[mode]], STD[:CH[mode]])
        ad = api.png_alpha_desc(alpha, (0.2, 0.4, 0.6)[:ch] if alpha == "over" else None, mode, 8)
        fd = api.png_filter_desc(filt)
        bgs = list(ad.background) if ad is not None else None
        slot = size[0] * size[1] * ch * es
        arena = torch.full((4096 + n * slot + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ins = [np.frombuffer(f, np.uint8) for f in files]
        st = (C.c_uint32 * n)()
        rc = L.debig_png_decode_batch_tensor_filter((C.c_void_p * n)(*[a.ctypes.data for a in ins]), (C.c_uint64 * n)(*[len(f) for f in files]),
                                                    arena.data_ptr() + 4096, None, st, None, n, 0, C.byref(d),
                                                    C.byref(ad) if ad is not None else None, C.byref(fd))
        N.check(rc, "debig_png_decode_batch_tensor_filter")
        a = arena.cpu().numpy()
        assert list(st) == [0] * 5 + [R.E_SIGNATURE] + [0] * 5
        assert (a[:4096] == 0xA5).all() and (a[4096 + n * slot:] == 0xA5).all() and (a[4096 + 5 * slot: 4096 + 6 * slot] == 0xA5).all()
        for i in (0, 4, 6, 9, 10):
            px = _host(api, files[i], mode if alpha == "straight" else WITH_ALPHA[mode], 8)[1]
            want = F.resize(px, size, filt, "float32", True, None, scale=list(d.scale), bias=list(d.bias), layout="hwc", alpha=alpha,
                            background=bgs)
            assert a[4096 + i * slot: 4096 + (i + 1) * slot].tobytes() == want.tobytes(), (filt, alpha, mode, i)


@pytest.mark.parametrize("alpha,mode,depth", [("straight", "rgb", 8), ("straight", "rgba", 16), ("over", "gray", 8),
                                              ("premultiplied", "gray_alpha", 8)])
def test_filter_bilinear_equals_the_call_without_the_argument(api, datas, alpha, mode, depth):
    """filter="bilinear" makes the old C calls; the new C call with filter == NULL or BILINEAR gives the same bytes"""
    import torch
    from debigulator_amd import _native as N

    ch = CH[mode]
    kw = dict(mean=MEAN[:ch], std=STD[:ch], alpha=alpha)
    st0, t0, inf0 = api.png_decode_batch_tensor(datas, (30, 26), mode=mode, depth=depth, dtype="float32", **kw)
    st1, t1, inf1 = api.png_decode_batch_tensor(datas, (30, 26), mode=mode, depth=depth, dtype="float32", filter="bilinear", **kw)
    assert st0 == st1 == [0] * len(datas) and inf0 == inf1 and _np(t0).tobytes() == _np(t1).tobytes()
    L = api._png_spec_lib()
    L.debig_png_decode_batch_tensor_filter.restype = C.c_int
    L.debig_png_decode_batch_tensor_filter.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    d = api.png_tensor_desc((30, 26), mode, depth, "float32", "chw", mean=MEAN[:ch], std=STD[:ch])[0]
    ad = api.png_alpha_desc(alpha, None, mode, depth)
    n = len(datas)
    ins = [np.frombuffer(f, np.uint8) for f in datas]
    for fd in (None, api.PngFilterDesc(filter=0)):
        out = torch.zeros_like(t0)
        torch.cuda.synchronize()
        st = (C.c_uint32 * n)()
        rc = L.debig_png_decode_batch_tensor_filter((C.c_void_p * n)(*[a.ctypes.data for a in ins]), (C.c_uint64 * n)(*[len(f) for f in datas]),
                                                    out.data_ptr(), None, st, None, n, 0, C.byref(d),
                                                    C.byref(ad) if ad is not None else None, C.byref(fd) if fd is not None else None)
        N.check(rc, "debig_png_decode_batch_tensor_filter")
        assert list(st) == st0 and _np(out).tobytes() == _np(t0).tobytes()
    # and the other filters do differ from it
    for filt in FILTERS:
        _, t2, _ = api.png_decode_batch_tensor(datas, (30, 26), mode=mode, depth=depth, dtype="float32", filter=filt, **kw)
        assert _np(t2).tobytes() != _np(t0).tobytes()


def test_nearest_is_the_source_sample_and_bicubic_overshoot_is_clamped(api):
    """a 0 / 255 checkerboard of 3-pixel blocks: nearest returns source samples only; bicubic enlarged 2.3 x stays inside
    [0, 255] although its sums leave it (the restatement's values before the clamp do), and equals the restatement"""
    y, x = np.mgrid[0:40, 0:56]
    img = np.repeat((np.where((x // 3 + y // 3) % 2 == 0, 255, 0).astype(np.uint8))[:, :, None], 3, axis=2)
    data = R.encode(img, 2, 8)
    st, t, _ = api.png_decode_batch_tensor([data], (92, 129), mode="rgb", dtype="uint", layout="hwc", filter="nearest")
    iy, ix = (2 * np.arange(92) + 1) * 40 // 184, (2 * np.arange(129) + 1) * 56 // 258
    assert st == [0] and np.array_equal(_np(t)[0], img[iy][:, ix])
    v = F.cubic_passes(img.astype(np.int64), 8, (92, 129), True)
    assert v.min() < 0 and v.max() > 255 << 21
    st, t, _ = api.png_decode_batch_tensor([data], (92, 129), mode="rgb", dtype="uint", layout="hwc", filter="bicubic")
    assert st == [0] and np.array_equal(_np(t)[0], F.resize(img, (92, 129), "bicubic", "uint"))
    st, t, _ = api.png_decode_batch_tensor([data], (40, 56), mode="rgb", dtype="uint", layout="hwc", filter="bicubic")
    assert st == [0] and np.array_equal(_np(t)[0], img)  # unscaled at P = 8: the image itself
