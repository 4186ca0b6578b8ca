"""debig_png_decode_batch_tensor on the MI355X (include/decode_png.h; api.png_decode_batch_tensor): the whole call, BIT FOR
BIT against the numpy restatement (tests/png_resize_ref.py) applied to the pixels of the existing host call
api.png_decode_batch -- every colour type and depth, Adam7, tRNS and tuned-route files at mixed sizes in ONE batch; every
dtype and both layouts; per-image boxes; identity size against png_decode_batch_device; every error status in the middle
of a batch with a sentinel-filled tensor; E_BOX; a batch of 256.  Nothing outside the repository is read."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_gpu_png_spec as G  # noqa: E402

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
CH = {"rgba": 4, "rgb": 3, "gray": 1, "gray_alpha": 2}
DTYPES = ["uint", "float32", "float16", "bfloat16"]


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A

    return A


@pytest.fixture(scope="module")
def datas():
    """every colour type / depth / Adam7 / tRNS combination (45 x 70) and tuned-route files (8-bit RGB / RGBA, not
    interlaced) of other sizes, interleaved"""
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


def _check(api, datas, size, mode="rgb", depth=8, dtype="float32", layout="chw", aa=True, boxes=None, norm=True, fill=None,
           expect=None):
    ch = CH[mode]
    kw = dict(mean=MEAN[:ch], std=STD[:ch]) if norm and dtype != "uint" else {}
    st, t, infos = api.png_decode_batch_tensor(datas, size, mode=mode, depth=depth, dtype=dtype, layout=layout, boxes=boxes,
                                               antialias=aa, fill=fill, **kw)
    d = api.png_tensor_desc(size, mode, depth, dtype, layout, antialias=aa, **kw)[0]
    got = _np(t)
    assert got.shape == ((len(datas), ch) + tuple(size) if layout == "chw" else (len(datas),) + tuple(size) + (ch,))
    for i, data in enumerate(datas):
        hst, px, hinf = _host(api, data, mode, depth)
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
        want = Z.resize(px, size, dtype, aa, box, scale=list(d.scale), bias=list(d.bias), layout=layout)
        assert got[i].dtype == want.dtype and got[i].shape == want.shape, (i, got[i].dtype, want.dtype)
        assert got[i].tobytes() == want.tobytes(), (i, hinf, size, mode, depth, dtype, layout, aa, box,
                                                    np.argwhere(got[i] != want)[:4])
    return st, got


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,depth", [("rgb", 8), ("rgba", 16), ("gray", 8), ("gray_alpha", 16), ("rgba", 8), ("rgb", 16)])
def test_mixed_batch_every_format_dtype_and_layout(api, datas, mode, depth, dtype, layout):
    st, _ = _check(api, datas, (32, 24), mode, depth, dtype, layout, aa=True)
    assert st == [0] * len(datas)
    _check(api, datas, (75, 50), mode, depth, dtype, layout, aa=False)


def test_flagship_shape_rgb8_to_224_chw_float32(api, datas):
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:500, 0:640]
    s = ((x[:, :, None] * 3 + y[:, :, None] * 2 + np.arange(3) * 40) // 3 % 256).astype(np.uint8)
    big = [R.encode((s + rng.integers(0, 9, size=s.shape)).astype(np.uint8)[: 500 - 37 * k, : 640 - 53 * k], 2, 8,
                    filters=lambda p, yy: yy % 5) for k in range(3)]
    big.append(R.encode(R.random_image(rng, 401, 333, 6, 16), 6, 16))
    st, got = _check(api, big + datas[:6], (224, 224))
    assert st == [0] * (len(big) + 6) and got.dtype == np.float32
    _check(api, big, (224, 224), dtype="bfloat16", layout="hwc")
    _check(api, big, (224, 224), mode="rgba", depth=16, dtype="float16", aa=False)


def test_per_image_boxes(api, datas):
    boxes = []
    for i, data in enumerate(datas):
        _, inf = api.png_info(data)
        w, h = inf["width"], inf["height"]
        k = i % 6
        boxes.append([None, (0, 0, 0, 0), (0, 0, max(w // 2, 1), max(h // 3, 1)), (w - max(w // 3, 1), h - max(h // 2, 1), max(w // 3, 1), max(h // 2, 1)),
                      (w - 1, 0, 1, h), (0, h - 1, w, 1)][k])
    for aa in (True, False):
        st, _ = _check(api, datas, (20, 16), "rgba", 8, "float32", "chw", aa=aa, boxes=boxes)
        assert st == [0] * len(datas)
        _check(api, datas, (20, 16), "rgb", 16, "uint", "hwc", aa=aa, boxes=boxes)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("mode,depth", [("rgba", 8), ("rgb", 16), ("gray", 8)])
def test_identity_size_equals_the_device_decode(api, mode, depth, layout):
    same = [d for _, d in G._all_formats()]  # all 45 x 70
    dev = api.png_decode_batch_device(same, mode=mode, depth=depth, layout=layout)
    for aa in (True, False):
        st, t, _ = api.png_decode_batch_tensor(same, (70, 45), mode=mode, depth=depth, dtype="uint", layout=layout, antialias=aa)
        got = _np(t)
        for i, (dst, dt, _) in enumerate(dev):
            assert st[i] == dst == 0
            assert np.array_equal(got[i], _np(dt)), (i, mode, depth, layout, aa)


@pytest.mark.parametrize("dtype,fill", [("float32", -7.5), ("uint", 0xA5), ("bfloat16", 3.0)])
def test_every_error_status_in_the_middle_of_a_batch(api, datas, dtype, fill):
    cases = G._error_files()
    good = datas[:4]
    batch = good[:2] + [d for _, d, _ in cases] + [b"not a png", datas[7][:40]] + good[2:]
    fmt_status = [s for s, _, _ in api.png_decode_batch(batch, mode="rgb", depth=8)]
    assert fmt_status[2: 2 + len(cases)] == [s for _, _, s in cases] and fmt_status[:2] == [0, 0] and fmt_status[-2:] == [0, 0]
    for layout in ("chw", "hwc"):
        st, _ = _check(api, batch, (19, 21), "rgb", 8, dtype, layout, fill=fill)  # statuses as _fmt gives them, slots hold the fill
        assert st == fmt_status
        assert sorted(set(st)) == sorted({0, R.E_SIGNATURE, R.E_CHUNK} | {s for _, _, s in cases})


def test_box_errors_beside_good_files(api, datas):
    rng = np.random.default_rng(3)
    tall = R.encode(R.random_image(rng, 3, 200, 0, 8), 0, 8)
    files = [datas[0], datas[1], tall, datas[2], datas[3], datas[4][:60], datas[5]]
    boxes = [None, (40, 0, 6, 5), None, (0, 0, 0, 9), (5, 6, 7, 8), (0, 0, 46, 1), (0, 69, 45, 1)]
    expect = [0, Z.E_BOX, Z.E_BOX, Z.E_BOX, 0, Z.E_BOX, 0]  # tall: 200 rows to 3 with antialias is a scale above 64
    st, _ = _check(api, files, (3, 9), "rgb", 8, "float32", "chw", boxes=boxes, fill=9.0, expect=expect)
    assert st == expect
    expect[2] = 0  # without antialias the tall file is resized
    _check(api, files, (3, 9), "rgb", 8, "float32", "chw", aa=False, boxes=boxes, fill=9.0, expect=expect)


def _fits(api, data, box):
    _, inf = api.png_info(data)
    return box[0] + box[2] <= inf["width"] and box[1] + box[3] <= inf["height"]


def test_batch_of_256(api, datas):
    batch = [datas[(7 * k) % len(datas)] for k in range(256)]
    boxes = [None if k % 3 else (k % 2, k % 5, 1 + k % 7, 1 + k % 4) for k in range(256)]  # (every file is at least 1 x 1 ... 5 x 300)
    boxes = [b if b is None or _fits(api, batch[k], b) else None for k, b in enumerate(boxes)]
    st, got = _check(api, batch, (48, 40), "rgb", 8, "float16", "chw", boxes=boxes)
    assert st == [0] * 256 and got.shape == (256, 3, 48, 40)


def test_nothing_outside_the_tensor_is_written(api, datas):
    """the C call on a slice in the middle of a sentinel-filled allocation"""
    import torch
    from debigulator_amd import _native as N

    L = api._png_spec_lib()
    L.debig_png_decode_batch_tensor.restype = C.c_int
    L.debig_png_decode_batch_tensor.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p]
    files = datas[:5] + [b"not a png"] + datas[5:9]
    n = len(files)
    d, ch, es = api.png_tensor_desc((33, 31), "rgb", 8, "float32", "hwc", MEAN[:3], STD[:3])
    slot = 33 * 31 * ch * es
    arena = torch.full((4096 + n * slot + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ins = [np.frombuffer(f, np.uint8) for f in files]
    st = (C.c_uint32 * n)()
    rc = L.debig_png_decode_batch_tensor((C.c_void_p * n)(*[a.ctypes.data for a in ins]), (C.c_uint64 * n)(*[len(f) for f in files]),
                                         arena.data_ptr() + 4096, None, st, None, n, 0, C.byref(d))
    N.check(rc, "debig_png_decode_batch_tensor")
    a = arena.cpu().numpy()
    assert list(st) == [0] * 5 + [R.E_SIGNATURE] + [0] * 4
    assert (a[:4096] == 0xA5).all() and (a[4096 + n * slot:] == 0xA5).all() and (a[4096 + 5 * slot: 4096 + 6 * slot] == 0xA5).all()
    for i in (0, 4, 6, 9):
        px = _host(api, files[i], "rgb", 8)[1]
        want = Z.resize(px, (33, 31), "float32", True, None, scale=list(d.scale), bias=list(d.bias), layout="hwc")
        assert a[4096 + i * slot: 4096 + (i + 1) * slot].tobytes() == want.tobytes(), i


def test_tensor_is_one_allocation_on_the_device(api, datas, gpu_device):
    import torch

    st, t, infos = api.png_decode_batch_tensor(datas[:5], (8, 12), device=gpu_device)
    assert t.device == torch.device(gpu_device) and t.is_contiguous() and tuple(t.shape) == (5, 3, 8, 12) and t.dtype == torch.float32
    st, t, _ = api.png_decode_batch_tensor(datas[:5], (8, 12), layout="hwc", dtype="uint", mode="gray")
    assert tuple(t.shape) == (5, 8, 12, 1) and t.dtype == torch.uint8
    st, t, _ = api.png_decode_batch_tensor([], (8, 12))
    assert st == [] and tuple(t.shape) == (0, 3, 8, 12)
    with pytest.raises(ValueError):
        api.png_decode_batch_tensor(datas[:2], (8, 12), mode="native")
    with pytest.raises(ValueError):
        api.png_decode_batch_tensor(datas[:2], (8, 12), device="cpu")
