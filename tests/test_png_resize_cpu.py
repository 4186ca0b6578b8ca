"""The resize arithmetic of debig_png_decode_batch_tensor (include/decode_png.h) without a GPU: the numpy restatement
(tests/png_resize_ref.py) against torch.nn.functional.interpolate in float64, the properties of the Q14 weights, the C
weights of the built library against the restatement, identity sizes, and the argument checks and E_BOX rules of the C call
(they are decided before any device work)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402

BAD_FORMAT, BAD_ARG = -1, -2
DUMMY = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced: the calls below never reach the device


class Box(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_decode_batch_tensor.restype = C.c_int
    L.debig_png_decode_batch_tensor.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p]
    L.debig_png_resize_weights.restype = C.c_uint32
    L.debig_png_resize_weights.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32), C.POINTER(C.c_int16), C.c_uint32]
    return L


# ---- the restatement against torch ----------------------------------------------------------------------------------------

TORCH_CASES = [  # (h, w), (H, W), box
    ((3, 5), (7, 9), None), ((5, 3), (2, 2), None), ((64, 48), (17, 23), None), ((100, 37), (37, 100), None),
    ((90, 120), (224, 224), None), ((300, 400), (64, 64), (10, 20, 333, 250)), ((1, 9), (4, 3), None), ((9, 1), (3, 4), None),
    ((1, 1), (5, 5), None), ((50, 60), (1, 1), None), ((41, 67), (41, 67), None), ((200, 200), (40, 70), (199, 0, 1, 200)),
    ((1024, 1024), (224, 224), None), ((1500, 40), (24, 40), None), ((77, 130), (200, 30), (3, 4, 120, 70)),
]


@pytest.mark.parametrize("P", [8, 16])
@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("src,size,box", TORCH_CASES)
def test_restatement_against_torch_interpolate(src, size, box, aa, P):
    """The bound is derived, not tuned.  A Q14 weight is the exact weight rounded to a multiple of 2^-14, so it is off by at
    most 2^-15; the correction that makes the weights sum to 16384 moves ONE tap by at most taps * 2^-15.  The weights of an
    axis are therefore off by at most taps * 2^-15 + taps * 2^-15 = taps * 2^-14 in total, and since every sample lies in
    [0, 1] of full scale, that is the most an axis changes a result.  Rounding Hq to 16 bits adds at most 2^-17 of full scale
    per horizontal result, which the vertical weights (sum 1) carry through unchanged: 2^-16 covers it.  Hence
        |restatement - float64 interpolate| <= (taps_x + taps_y) * 2^-14 + 2^-16   (of full scale).
    torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=aa) in float64 is the reference."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(src[0] * 7 + src[1] + size[0])
    full = (1 << P) - 1
    px = rng.integers(0, full + 1, size=(src[0], src[1], 2), dtype=np.uint16).astype(np.uint8 if P == 8 else np.uint16)
    px[: src[0] // 2, : src[1] // 3] = full
    v, p = Z.resize_int(px, size, aa, box)
    assert p == P
    crop = px if box is None else px[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
    t = torch.from_numpy(crop.astype(np.float64) / full).permute(2, 0, 1)[None]
    ref = torch.nn.functional.interpolate(t, size=size, mode="bilinear", align_corners=False, antialias=aa)[0].permute(1, 2, 0).numpy()
    got = v.astype(np.float64) / float(1 << (30 - P)) / full
    taps_x = max(len(w) for _, w in Z.axis(crop.shape[1], size[1], aa))
    taps_y = max(len(w) for _, w in Z.axis(crop.shape[0], size[0], aa))
    bound = (taps_x + taps_y) * 2.0 ** -14 + 2.0 ** -16
    err = float(np.abs(got - ref).max())
    print(f"taps {taps_x}+{taps_y}: max |delta| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound, taps_x, taps_y)


# ---- the weights ------------------------------------------------------------------------------------------------------------

SWEEP = ([(cl, L) for cl in (1, 2, 3, 5, 7, 13, 64, 97, 101, 128, 257, 1024) for L in (1, 2, 3, 7, 16, 31, 64, 97, 224) if cl <= 64 * L] +
         [(64 * L, L) for L in (1, 2, 3, 5, 17)] + [(64 * L - 1, L) for L in (1, 3, 17)] + [(1500, 24), (4099, 127), (16411, 16384)])


@pytest.mark.parametrize("aa", [True, False])
def test_weights_are_non_negative_sum_to_one_and_contiguous(aa):
    for cl, L in SWEEP:
        prev_first, prev_end = 0, 0
        for X in ([0, 1, L // 2, L - 2, L - 1] if L > 512 else range(L)):
            if not 0 <= X < L:
                continue
            f, w = Z.taps(cl, L, aa, X)
            assert all(x >= 0 for x in w) and sum(w) == Z.ONE, (cl, L, X, w)
            assert 0 <= f and f + len(w) <= cl and 1 <= len(w) <= 129, (cl, L, X, f, len(w))
            assert f >= prev_first and f + len(w) >= prev_end, (cl, L, X)  # the windows move right: a tile's span is first..last
            prev_first, prev_end = f, f + len(w)


@pytest.mark.parametrize("aa", [True, False])
def test_c_weights_equal_the_restatement(lib, aa):
    w = (C.c_int16 * 132)()
    first = C.c_uint32()
    for cl, L in SWEEP:
        for X in ([0, 1, L // 2, L - 2, L - 1] if L > 512 else range(L)):
            if not 0 <= X < L:
                continue
            n = lib.debig_png_resize_weights(cl, L, int(aa), X, C.byref(first), w, 132)
            f, want = Z.taps(cl, L, aa, X)
            assert n == len(want) and first.value == f and list(w[:n]) == want, (cl, L, X)
    # refused: a scale above 64 with antialias, X outside the axis, zero lengths, too small a buffer
    assert lib.debig_png_resize_weights(65, 1, 1, 0, C.byref(first), w, 132) == 0
    assert lib.debig_png_resize_weights(65, 1, 0, 0, C.byref(first), w, 132) in (1, 2)
    assert lib.debig_png_resize_weights(10, 5, 1, 5, C.byref(first), w, 132) == 0
    assert lib.debig_png_resize_weights(0, 5, 1, 0, C.byref(first), w, 132) == 0
    assert lib.debig_png_resize_weights(5, 0, 1, 0, C.byref(first), w, 132) == 0
    assert lib.debig_png_resize_weights(100, 10, 1, 3, C.byref(first), w, 3) == 0


@pytest.mark.parametrize("P", [8, 16])
def test_identity_size_is_exactly_the_crop(P):
    rng = np.random.default_rng(P)
    px = rng.integers(0, 1 << P, size=(37, 53, 4), dtype=np.uint16).astype(np.uint8 if P == 8 else np.uint16)
    for aa in (True, False):
        assert np.array_equal(Z.resize(px, (37, 53), "uint", aa), px)
        assert np.array_equal(Z.resize(px, (20, 11), "uint", aa, box=(5, 6, 11, 20)), px[6:26, 5:16])
        f = Z.resize(px, (37, 53), "float32", aa)
        assert np.array_equal(f, (px.astype(np.float32) * np.float32(1 << (30 - P))) * Z.affine(P, [1] * 4, [0] * 4)[0][0])
        assert float(np.abs(f - px / float((1 << P) - 1)).max()) < 2e-7


def test_bfloat16_rounding_is_to_nearest_even():
    f = np.array([1.0, 1.00390625, 1.01171875, -2.5, 3.4e38, 0.0], np.float32)  # ties: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert list(Z.bf16_bits(f)) == [0x3F80, 0x3F80, 0x3F82, 0xC020, 0x7F80, 0x0000]


# ---- the C call's checks (no GPU: everything below returns before any device work) ---------------------------------------

class Desc(C.Structure):
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("out_format", C.c_uint32), ("out_layout", C.c_uint32),
                ("dtype", C.c_uint32), ("resize_flags", C.c_uint32), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


def _desc(**kw):
    d = Desc(out_w=8, out_h=8, out_format=1, out_layout=1, dtype=1, resize_flags=1)
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    for k, v in kw.items():
        if k in ("scale", "bias"):
            for j, x in enumerate(v):
                getattr(d, k)[j] = x
        else:
            setattr(d, k, v)
    return d


def _call(lib, files, desc, out=DUMMY, boxes=None):
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    st = (C.c_uint32 * n)(*[0xABCD] * n)
    bx = (Box * n)(*[Box(*b) for b in boxes]) if boxes is not None else None
    rc = lib.debig_png_decode_batch_tensor(ins, sizes, out, bx, st, None, n, 0, C.byref(desc) if desc is not None else None)
    return rc, list(st)


@pytest.mark.parametrize("kw,want", [
    (dict(out_format=4), BAD_FORMAT), (dict(out_format=0x20), BAD_FORMAT), (dict(out_format=0x24), BAD_FORMAT),
    (dict(out_format=0x30), BAD_FORMAT), (dict(out_format=0x101), BAD_FORMAT), (dict(out_layout=2), BAD_FORMAT),
    (dict(dtype=4), BAD_ARG), (dict(resize_flags=2), BAD_ARG), (dict(resize_flags=0x80000001), BAD_ARG),
    (dict(out_w=0), BAD_ARG), (dict(out_h=0), BAD_ARG), (dict(out_w=16385), BAD_ARG), (dict(out_h=16385), BAD_ARG),
    (dict(scale=[1.0, float("inf")]), BAD_ARG), (dict(bias=[0.0, 0.0, float("nan")]), BAD_ARG),
    (dict(scale=[float("-inf")]), BAD_ARG),
])
def test_bad_descriptors_are_refused_before_any_file(lib, kw, want):
    rc, st = _call(lib, [b"not a png"] * 2, _desc(**kw))
    assert rc == want and st == [0xABCD] * 2


def test_bad_pointers_are_refused_before_any_file(lib):
    assert _call(lib, [b"not a png"], None) == (BAD_ARG, [0xABCD])
    assert _call(lib, [b"not a png"], _desc(), out=None) == (BAD_ARG, [0xABCD])
    for off in (1, 4, 8, 15):
        assert _call(lib, [b"not a png"], _desc(), out=DUMMY + off) == (BAD_ARG, [0xABCD])
    assert lib.debig_png_decode_batch_tensor(None, None, None, None, None, None, 0, 0, None) == 0  # n == 0: nothing to do


def test_non_finite_scale_is_ignored_for_the_integer_dtype(lib):
    rc, st = _call(lib, [b"not a png"], _desc(dtype=0, scale=[float("nan")]))
    assert rc == 0 and st == [R.E_SIGNATURE]


def test_box_rules(lib):
    rng = np.random.default_rng(1)
    png = R.encode(R.random_image(rng, 40, 30, 2, 8), 2, 8)  # 40 wide, 30 high
    st, _, inf = R.decode(png)
    assert st == R.OK and (inf["width"], inf["height"]) == (40, 30)
    bad = [(0, 0, 5, 0), (0, 0, 0, 5), (36, 0, 5, 5), (0, 26, 5, 5), (40, 0, 1, 1), (0xFFFFFFFF, 0, 2, 2), (1, 0, 0xFFFFFFFF, 1),
           (0, 0xFFFFFFF0, 1, 0x20)]
    files = [png] * len(bad) + [b"not a png", png[:60], png[:60]]
    boxes = bad + [(0, 0, 5, 0), (0, 0, 41, 1), (0, 0, 40, 30)]
    rc, st = _call(lib, files, _desc(), boxes=boxes)
    # a broken file without a valid IHDR keeps its own status; E_BOX outranks what comes later in a file; a good box does not
    assert rc == 0 and st == [Z.E_BOX] * len(bad) + [R.E_SIGNATURE, Z.E_BOX, R.E_CHUNK]
    for b, f in zip(boxes, files):
        if f is png:
            assert not Z.box_ok(b, 40, 30, (8, 8), True)
    # antialias beyond a scale of 64 on either axis; the same boxes pass the box rule without antialias
    tall = R.encode(R.random_image(rng, 3, 200, 0, 8), 0, 8)
    wide = R.encode(R.random_image(rng, 200, 3, 0, 8), 0, 8)
    rc, st = _call(lib, [tall, wide, tall], _desc(out_w=3, out_h=3, out_format=2), boxes=[(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 3, 193)])
    assert rc == 0 and st == [Z.E_BOX] * 3
    rc, st = _call(lib, [tall[:50]], _desc(out_w=3, out_h=3, out_format=2, resize_flags=0))
    assert rc == 0 and st == [R.E_CHUNK]  # without antialias the box is fine: the truncated file's own status


def test_python_arguments():
    from debigulator_amd import api

    with pytest.raises(ValueError):
        api.png_tensor_desc((8, 8), mode="native")
    with pytest.raises(ValueError):
        api.png_tensor_desc((8, 8), depth="native")
    with pytest.raises(ValueError):
        api.png_tensor_desc((8, 8), dtype="float64")
    with pytest.raises(ValueError):
        api.png_tensor_desc((8, 8), dtype="uint16", depth=8)
    with pytest.raises(ValueError):
        api.png_tensor_desc((0, 8))
    with pytest.raises(ValueError):
        api.png_tensor_desc((8, 8), mean=[0.5, 0.5], std=[1, 1])
    with pytest.raises(ValueError):
        api.png_tensor_desc((8, 8), std=[1, 0, 1])
    d, ch, es = api.png_tensor_desc((224, 200), mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
    assert (d.out_h, d.out_w, d.out_format, d.out_layout, d.dtype, d.resize_flags, ch, es) == (224, 200, 1, 1, 1, 1, 3, 4)
    assert d.scale[1] == np.float32(1 / 0.224) and d.bias[2] == np.float32(-0.406 / 0.225)
    assert api.png_tensor_desc((8, 8), mode="gray_alpha", depth=16, dtype="uint16", layout="hwc", antialias=False)[1:] == (2, 2)
    assert api.PNG_STATUS[14] == "box"


def test_symbols_are_exported(lib):
    from debigulator_amd import _native as N

    out = os.popen(f"nm -D --defined-only {N.LIB_PATH}").read()
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"debig_png_decode_batch_tensor", "debig_png_resize_weights", "debig_hip_png_resize_batch"} <= syms
