"""debig_png_decode_batch_tensor_alpha on the MI355X (include/decode_png.h; api.png_decode_batch_tensor(alpha=...)): the whole
call, BIT FOR BIT against the numpy restatement (tests/png_alpha_ref.py) applied to the pixels of the existing host call
api.png_decode_batch(mode="rgba" | "gray_alpha") -- every colour type and depth, Adam7, tRNS and tuned-route files at mixed
sizes in ONE batch; OVER and PREMULTIPLIED, every dtype, both layouts; per-image boxes; the 224 x 224 flagship shape; files
without alpha against today's call for three backgrounds; every error status in the middle of a batch with a
sentinel-filled tensor; nothing outside the tensor written; alpha="straight" against the old call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_alpha_ref as A  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_gpu_png_spec as G  # noqa: E402

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
CH = {"rgba": 4, "rgb": 3, "gray": 1, "gray_alpha": 2}
SRC = {"rgb": "rgba", "gray": "gray_alpha", "rgba": "rgba", "gray_alpha": "gray_alpha"}  # the format decoded with its alpha
DTYPES = ["uint", "float32", "float16", "bfloat16"]
BACKGROUNDS = [None, 0.0, (0.25, 1.0, 0.6)]


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


def _bg(background, mode, depth):
    ch = CH[mode]
    if background is not None and hasattr(background, "__len__"):
        background = background[:ch]
    return background, A.background_samples(background, ch, depth)


def _check(api, datas, size, alpha, mode, depth=8, dtype="float32", layout="chw", aa=True, boxes=None, background=None,
           fill=None, expect=None):
    ch = CH[mode]
    kw = dict(mean=MEAN[:ch], std=STD[:ch]) if dtype != "uint" else {}
    akw = {}
    bgs = None
    if alpha == "over":
        background, bgs = _bg(background, mode, depth)
        akw = dict(background=background)
    st, t, infos = api.png_decode_batch_tensor(datas, size, mode=mode, depth=depth, dtype=dtype, layout=layout, boxes=boxes,
                                               antialias=aa, fill=fill, alpha=alpha, **akw, **kw)
    d = api.png_tensor_desc(size, mode, depth, dtype, layout, antialias=aa, **kw)[0]
    got = _np(t)
    assert got.shape == ((len(datas), ch) + tuple(size) if layout == "chw" else (len(datas),) + tuple(size) + (ch,))
    for i, data in enumerate(datas):
        hst, px, hinf = _host(api, data, SRC[mode], depth)
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
        want = A.resize_alpha(px, size, alpha, dtype, aa, box, background=bgs, scale=list(d.scale), bias=list(d.bias), layout=layout)
        assert got[i].dtype == want.dtype and got[i].shape == want.shape, (i, got[i].dtype, want.dtype)
        assert got[i].tobytes() == want.tobytes(), (i, hinf, size, alpha, mode, depth, dtype, layout, aa, box, bgs,
                                                    np.argwhere(got[i] != want)[:4])
    return st, got


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("alpha,mode,depth", [("over", "rgb", 8), ("over", "rgb", 16), ("over", "gray", 8), ("over", "gray", 16),
                                              ("premultiplied", "rgba", 8), ("premultiplied", "rgba", 16),
                                              ("premultiplied", "gray_alpha", 8), ("premultiplied", "gray_alpha", 16)])
def test_mixed_batch_every_mode_format_dtype_and_layout(api, datas, alpha, mode, depth, dtype, layout):
    k = DTYPES.index(dtype) + (layout == "hwc")
    st, _ = _check(api, datas, (32, 24), alpha, mode, depth, dtype, layout, aa=True, background=BACKGROUNDS[k % 3])
    assert st == [0] * len(datas)
    _check(api, datas, (75, 50), alpha, mode, depth, dtype, layout, aa=False, background=BACKGROUNDS[(k + 1) % 3])


def _flagship_files():
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:500, 0:640]
    s = ((x[:, :, None] * 3 + y[:, :, None] * 2 + np.arange(4) * 40) // 3 % 256).astype(np.uint8)
    s[:, :, 3] = np.where((x // 40 + y // 25) % 3 == 0, 0, np.where((x // 40 + y // 25) % 3 == 1, 255, s[:, :, 3]))  # hard edges
    big = [R.encode(np.ascontiguousarray((s + rng.integers(0, 9, size=s.shape)).astype(np.uint8)[: 500 - 37 * k, : 640 - 53 * k]), 6, 8,
                    filters=lambda p, yy: yy % 5) for k in range(3)]
    big.append(R.encode(R.random_image(rng, 401, 333, 6, 16), 6, 16))
    big.append(R.encode(R.random_image(rng, 300, 280, 4, 8), 4, 8))
    return big


def test_flagship_shape_over_white_to_224_chw_float32(api, datas):
    big = _flagship_files()
    st, got = _check(api, big + datas[:6], (224, 224), "over", "rgb")
    assert st == [0] * (len(big) + 6) and got.dtype == np.float32 and got.shape[1:] == (3, 224, 224)
    _check(api, big, (224, 224), "over", "rgb", dtype="bfloat16", layout="hwc", background=(0.0, 0.5, 1.0))
    _check(api, big, (224, 224), "premultiplied", "rgba", depth=16, dtype="float16", aa=False)
    _check(api, big, (224, 224), "over", "gray", depth=16, dtype="uint", background=0.5)


def test_per_image_boxes(api, datas):
    boxes = []
    for i, data in enumerate(datas):
        _, inf = api.png_info(data)
        w, h = inf["width"], inf["height"]
        k = i % 6
        boxes.append([None, (0, 0, 0, 0), (0, 0, max(w // 2, 1), max(h // 3, 1)), (w - max(w // 3, 1), h - max(h // 2, 1), max(w // 3, 1), max(h // 2, 1)),
                      (w - 1, 0, 1, h), (0, h - 1, w, 1)][k])
    for aa in (True, False):
        st, _ = _check(api, datas, (20, 16), "over", "rgb", 8, "float32", "chw", aa=aa, boxes=boxes, background=(1.0, 0.0, 0.5))
        assert st == [0] * len(datas)
        _check(api, datas, (20, 16), "premultiplied", "rgba", 16, "uint", "hwc", aa=aa, boxes=boxes)
        _check(api, datas, (20, 16), "over", "gray", 16, "float16", "hwc", aa=aa, boxes=boxes, background=0.3)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_files_without_alpha_equal_todays_rgb_call(api, datas, dtype, layout):
    """no alpha channel, no tRNS: compositing changes nothing, whatever the background -- byte for byte the old call"""
    plain = [d for d in datas if api.png_info(d)[1]["color_type"] in (0, 2, 3) and not api.png_info(d)[1]["has_trns"]]
    assert len(plain) >= 12
    kw = dict(mean=MEAN[:3], std=STD[:3]) if dtype != "uint" else {}
    for depth in (8, 16):
        st0, t0, inf0 = api.png_decode_batch_tensor(plain, (40, 28), mode="rgb", depth=depth, dtype=dtype, layout=layout, **kw)
        assert st0 == [0] * len(plain)
        for background in BACKGROUNDS:
            st, t, inf = api.png_decode_batch_tensor(plain, (40, 28), mode="rgb", depth=depth, dtype=dtype, layout=layout,
                                                     alpha="over", background=background, **kw)
            assert st == st0 and inf == inf0
            assert _np(t).tobytes() == _np(t0).tobytes(), (depth, dtype, layout, background)
    st0, t0, _ = api.png_decode_batch_tensor(plain, (40, 28), mode="rgba", dtype=dtype, layout=layout)
    st, t, _ = api.png_decode_batch_tensor(plain, (40, 28), mode="rgba", dtype=dtype, layout=layout, alpha="premultiplied")
    assert st == st0 and _np(t).tobytes() == _np(t0).tobytes()


@pytest.mark.parametrize("alpha,mode", [("over", "rgb"), ("premultiplied", "rgba"), ("over", "gray")])
@pytest.mark.parametrize("dtype,fill", [("float32", -7.5), ("uint", 0xA5), ("bfloat16", 3.0)])
def test_every_error_status_in_the_middle_of_a_batch(api, datas, dtype, fill, alpha, mode):
    cases = G._error_files()
    good = datas[:4]
    batch = good[:2] + [d for _, d, _ in cases] + [b"not a png", datas[7][:40]] + good[2:]
    fmt_status = [s for s, _, _ in api.png_decode_batch(batch, mode="rgb", depth=8)]
    assert fmt_status[2: 2 + len(cases)] == [s for _, _, s in cases] and fmt_status[:2] == [0, 0] and fmt_status[-2:] == [0, 0]
    for layout in ("chw", "hwc"):
        st, _ = _check(api, batch, (19, 21), alpha, mode, 8, dtype, layout, fill=fill, background=(0.1, 0.9, 0.4))
        assert st == fmt_status  # statuses as the tensor call gives them; the failed slots hold the fill
        assert sorted(set(st)) == sorted({0, R.E_SIGNATURE, R.E_CHUNK} | {s for _, _, s in cases})


def test_box_errors_beside_good_files(api, datas):
    rng = np.random.default_rng(3)
    tall = R.encode(R.random_image(rng, 3, 200, 4, 8), 4, 8)
    files = [datas[0], datas[1], tall, datas[2], datas[3], datas[4][:60], datas[5]]
    boxes = [None, (40, 0, 6, 5), None, (0, 0, 0, 9), (5, 6, 7, 8), (0, 0, 46, 1), (0, 69, 45, 1)]
    expect = [0, Z.E_BOX, Z.E_BOX, Z.E_BOX, 0, Z.E_BOX, 0]  # tall: 200 rows to 3 with antialias is a scale above 64
    st, _ = _check(api, files, (3, 9), "over", "rgb", 8, "float32", "chw", boxes=boxes, fill=9.0, expect=expect)
    assert st == expect
    expect[2] = 0  # without antialias the tall file is resized
    _check(api, files, (3, 9), "over", "rgb", 8, "float32", "chw", aa=False, boxes=boxes, fill=9.0, expect=expect)


def test_nothing_outside_the_tensor_is_written(api, datas):
    """the C call on a slice in the middle of a sentinel-filled allocation"""
    import torch
    from debigulator_amd import _native as N

    L = api._png_spec_lib()
    L.debig_png_decode_batch_tensor_alpha.restype = C.c_int
    L.debig_png_decode_batch_tensor_alpha.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    files = datas[:5] + [b"not a png"] + datas[5:9] + _flagship_files()[:1]
    n = len(files)
    for alpha, mode, size in (("over", "rgb", (33, 31)), ("premultiplied", "gray_alpha", (70, 45)), ("over", "gray", (9, 200))):
        d, ch, es = api.png_tensor_desc(size, mode, 8, "float32", "hwc", MEAN[:CH[mode]], STD[:CH[mode]])
        ad = api.png_alpha_desc(alpha, (0.2, 0.4, 0.6)[:ch] if alpha == "over" else None, mode, 8)
        bgs = list(ad.background)
        slot = size[0] * size[1] * ch * es
        arena = torch.full((4096 + n * slot + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ins = [np.frombuffer(f, np.uint8) for f in files]
        st = (C.c_uint32 * n)()
        rc = L.debig_png_decode_batch_tensor_alpha((C.c_void_p * n)(*[a.ctypes.data for a in ins]), (C.c_uint64 * n)(*[len(f) for f in files]),
                                                   arena.data_ptr() + 4096, None, st, None, n, 0, C.byref(d), C.byref(ad))
        N.check(rc, "debig_png_decode_batch_tensor_alpha")
        a = arena.cpu().numpy()
        assert list(st) == [0] * 5 + [R.E_SIGNATURE] + [0] * 5
        assert (a[:4096] == 0xA5).all() and (a[4096 + n * slot:] == 0xA5).all() and (a[4096 + 5 * slot: 4096 + 6 * slot] == 0xA5).all()
        for i in (0, 4, 6, 9, 10):
            px = _host(api, files[i], SRC[mode], 8)[1]
            want = A.resize_alpha(px, size, alpha, "float32", True, None, background=bgs, scale=list(d.scale), bias=list(d.bias), layout="hwc")
            assert a[4096 + i * slot: 4096 + (i + 1) * slot].tobytes() == want.tobytes(), (alpha, mode, i)


@pytest.mark.parametrize("mode,depth", [("rgb", 8), ("rgba", 16), ("gray", 8), ("gray_alpha", 8)])
def test_alpha_straight_equals_the_old_call(api, datas, mode, depth):
    """alpha="straight" makes the old C call; the new C call with alpha == NULL or mode STRAIGHT gives the same bytes"""
    import torch
    from debigulator_amd import _native as N

    ch = CH[mode]
    kw = dict(mean=MEAN[:ch], std=STD[:ch])
    st0, t0, inf0 = api.png_decode_batch_tensor(datas, (30, 26), mode=mode, depth=depth, dtype="float32", **kw)
    st1, t1, inf1 = api.png_decode_batch_tensor(datas, (30, 26), mode=mode, depth=depth, dtype="float32", alpha="straight", **kw)
    assert st0 == st1 == [0] * len(datas) and inf0 == inf1 and _np(t0).tobytes() == _np(t1).tobytes()
    L = api._png_spec_lib()
    L.debig_png_decode_batch_tensor_alpha.restype = C.c_int
    L.debig_png_decode_batch_tensor_alpha.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    d = api.png_tensor_desc((30, 26), mode, depth, "float32", "chw", **kw)[0]
    n = len(datas)
    ins = [np.frombuffer(f, np.uint8) for f in datas]
    for ad in (None, api.PngAlphaDesc(mode=0, background=(C.c_uint16 * 4)(1, 2, 3, 4))):
        out = torch.zeros_like(t0)
        torch.cuda.synchronize()
        st = (C.c_uint32 * n)()
        rc = L.debig_png_decode_batch_tensor_alpha((C.c_void_p * n)(*[a.ctypes.data for a in ins]), (C.c_uint64 * n)(*[len(f) for f in datas]),
                                                   out.data_ptr(), None, st, None, n, 0, C.byref(d), C.byref(ad) if ad is not None else None)
        N.check(rc, "debig_png_decode_batch_tensor_alpha")
        assert list(st) == st0 and _np(out).tobytes() == _np(t0).tobytes()


def test_transparency_is_honoured_where_the_old_call_shows_hidden_colours(api):
    """a fully transparent RGBA file with garbage under its alpha: OVER gives the background exactly, PREMULTIPLIED zeros"""
    rng = np.random.default_rng(11)
    img = R.random_image(rng, 90, 70, 6, 8)
    img[:, :, 3] = 0
    data = R.encode(img, 6, 8)
    st, t, _ = api.png_decode_batch_tensor([data], (24, 24), mode="rgb", dtype="uint", layout="hwc", alpha="over", background=(1.0, 0.0, 0.5))
    assert st == [0] and (_np(t)[0] == np.array([255, 0, 128], np.uint8)).all()
    st, t, _ = api.png_decode_batch_tensor([data], (24, 24), mode="rgba", dtype="uint", layout="hwc", alpha="premultiplied")
    assert st == [0] and (_np(t) == 0).all()
    st, t, _ = api.png_decode_batch_tensor([data], (24, 24), mode="rgb", dtype="uint", layout="hwc")
    assert st == [0] and _np(t).std() > 10  # the old call: the colours stored under the transparent pixels
