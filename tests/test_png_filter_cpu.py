"""The filters of debig_png_decode_batch_tensor_filter (include/decode_png.h) without a GPU: the host's weight tables against
the numpy restatement (tests/png_filter_ref.py) over the whole sweep the header quotes, the properties of the bicubic rule,
the argument checks and the E_BOX edges of the C call (decided before any device work), nearest against torch's
"nearest-exact", and the closeness of the integer bicubic arithmetic to torch's float64 bicubic.

Closeness, measured on the fixed cases of test_bicubic_is_close_to_torch_float64 (maximum over shapes, contents and both
antialias settings, in output levels of full scale M = 2^P - 1): P = 8: 0.0432 for the float32 output and 1 level for UINT
against the rounded reference; P = 16: 11.61 and 12 levels -- the Q14 quantisation of the weights and the 15-bit intermediate.
The test asserts twice the measured values: 0.0864 / 2 (P = 8) and 23.22 / 24 (P = 16); a wrong tap, sign or clamp errs by far
more (torch's a = -0.75 variant alone differs by 15 - 31 levels of 255)."""
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
from test_png_alpha_cpu import AlphaDesc, Desc, BAD_ARG, BAD_FORMAT, DUMMY, RGB, RGBA, GRAY, _alpha, _desc  # noqa: E402

# twice the maxima measured on CASES below (module docstring): (float32 output in levels, UINT output in levels)
BOUNDS = {8: (2 * 0.0432, 2 * 1), 16: (2 * 11.61, 2 * 12)}


class FilterDesc(C.Structure):  # include/decode_png.h: debig_png_filter_desc
    _fields_ = [("filter", C.c_uint32), ("reserved", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_decode_batch_tensor_filter.restype = C.c_int
    L.debig_png_decode_batch_tensor_filter.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.debig_png_decode_batch_tensor_alpha.restype = C.c_int
    L.debig_png_decode_batch_tensor_alpha.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.debig_png_decode_batch_tensor.restype = C.c_int
    L.debig_png_decode_batch_tensor.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p]
    for f in (L.debig_png_resize_weights_filter, L.debig_png_resize_weights):
        f.restype = C.c_uint32
    L.debig_png_resize_weights_filter.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_uint32), C.POINTER(C.c_int16), C.c_uint32]
    L.debig_png_resize_weights.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32), C.POINTER(C.c_int16), C.c_uint32]
    return L


# ---- the weight rules ------------------------------------------------------------------------------------------------------

def _host_taps(lib, filt, cl, L, aa, X, cap=129):
    first = C.c_uint32(0xFFFFFFFF)
    w = (C.c_int16 * 129)()
    n = lib.debig_png_resize_weights_filter(filt, cl, L, aa, X, C.byref(first), w, cap)
    return (first.value, list(w[:n])) if n else None


def _sweep_pairs():
    pairs = [(cl, L) for cl in range(1, 70) for L in range(1, 70)]
    rng = np.random.default_rng(12)
    while len(pairs) < 69 * 69 + 300:  # larger pairs: shrinking up to the limit, enlarging, nearly equal
        L = int(rng.integers(1, 400))
        cl = int(rng.integers(1, 32 * L + 1)) if rng.integers(0, 2) else int(rng.integers(1, 3000))
        pairs.append((cl, L))
    return pairs + [(32 * L, L) for L in (1, 2, 3, 7, 64, 100)]  # the edge of the antialiased scale


def test_bicubic_weight_sweep_host_against_restatement(lib):
    """every cl, L in 1 .. 69, both antialias settings, every X; 300 larger pairs; cl = 32 L: the host's table is the
    restatement's, sum 16384, T > 0 (a table exists), at most 129 taps, sum |w| <= 32768, identity at cl == L"""
    max_abs, max_at, max_taps, lo, hi = 0, None, 0, 0, 0
    for cl, L in _sweep_pairs():
        for aa in (0, 1):
            if aa and cl > 32 * L:
                assert _host_taps(lib, F.BICUBIC, cl, L, aa, 0) is None
                continue
            xs = range(L) if L <= 69 else sorted({0, 1, 2, L // 3, L // 2, L - 3, L - 2, L - 1})
            for X in xs:
                want = F.taps(F.BICUBIC, cl, L, aa, X)
                assert want is not None, (cl, L, aa, X)  # T > 0 and sum |w| <= 32768
                got = _host_taps(lib, F.BICUBIC, cl, L, aa, X)
                assert got == want, (cl, L, aa, X, got, want)
                f, w = want
                assert sum(w) == F.ONE and 1 <= len(w) <= 129 and f + len(w) <= cl
                s = sum(abs(x) for x in w)
                if s > max_abs:
                    max_abs, max_at = s, (cl, L, aa, X)
                max_taps, lo, hi = max(max_taps, len(w)), min(lo, min(w)), max(hi, max(w))
                if cl == L:
                    assert [x for x in w if x] == [F.ONE] and f + w.index(F.ONE) == X
    print(f"bicubic sweep: max sum |w| {max_abs} at (cl, L, aa, X) = {max_at}, max taps {max_taps}, weights in [{lo}, {hi}]")
    assert max_abs <= 32768 and max_taps <= 129


def test_nearest_and_bilinear_tables(lib):
    for cl, L in [(cl, L) for cl in range(1, 40) for L in range(1, 40)] + [(5000, 3), (3, 5000), (12345, 16384), (1 << 31, 16384)]:
        for aa in (0, 1):
            for X in (range(L) if L < 100 else (0, 1, L // 2, L - 1)):
                assert _host_taps(lib, F.NEAREST, cl, L, aa, X) == (((2 * X + 1) * cl) // (2 * L), [F.ONE])
                if cl <= 64 * L and cl < 1 << 20:
                    first, w = C.c_uint32(0), (C.c_int16 * 129)()
                    n = lib.debig_png_resize_weights(cl, L, aa, X, C.byref(first), w, 129)
                    assert _host_taps(lib, F.BILINEAR, cl, L, aa, X) == (first.value, list(w[:n])) == Z.taps(cl, L, aa, X)
    # the failures of debig_png_resize_weights, an unknown filter, a table that is too short
    for filt in (F.BICUBIC, F.NEAREST):
        assert _host_taps(lib, filt, 0, 4, 1, 0) is None and _host_taps(lib, filt, 4, 0, 1, 0) is None
        assert _host_taps(lib, filt, 4, 16385, 1, 0) is None and _host_taps(lib, filt, 4, 4, 1, 4) is None
        assert _host_taps(lib, filt, 9, 4, 1, 1, cap=0) is None
    assert _host_taps(lib, 3, 4, 4, 1, 0) is None and _host_taps(lib, 0xFFFFFFFF, 4, 4, 1, 0) is None
    n = len(F.taps(F.BICUBIC, 9, 4, 1, 1)[1])
    assert _host_taps(lib, F.BICUBIC, 9, 4, 1, 1, cap=n - 1) is None and _host_taps(lib, F.BICUBIC, 9, 4, 1, 1, cap=n) == F.taps(F.BICUBIC, 9, 4, 1, 1)
    assert _host_taps(lib, F.BICUBIC, 65, 2, 1, 0) is None and _host_taps(lib, F.BICUBIC, 64, 2, 1, 0) is not None
    assert _host_taps(lib, F.BICUBIC, 65, 2, 0, 0) is not None and _host_taps(lib, F.NEAREST, 6500, 2, 1, 0) is not None


# ---- the C call's checks (no GPU: everything below returns before any device work) ---------------------------------------

def _filter(filt, reserved=0):
    return FilterDesc(filter=filt, reserved=reserved)


def _call(lib, files, desc, alpha, filt, out=DUMMY, boxes=None):
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    st = (C.c_uint32 * n)(*[0xABCD] * n)
    bx = (C.c_uint32 * (4 * n))(*[v for b in boxes for v in b]) if boxes is not None else None
    rc = lib.debig_png_decode_batch_tensor_filter(ins, sizes, out, bx, st, None, n, 0, C.byref(desc) if desc is not None else None,
                                                  C.byref(alpha) if alpha is not None else None,
                                                  C.byref(filt) if filt is not None else None)
    return rc, list(st)


def test_bad_filter_descriptors_are_refused_before_any_file(lib):
    for filt in (_filter(3), _filter(0xFFFFFFFF), _filter(F.BICUBIC, 1), _filter(F.BILINEAR, 0x80000000), _filter(F.NEAREST, 2)):
        for alpha, kw in ((None, {}), (_alpha(A.OVER), {}), (_alpha(A.PREMULTIPLIED), dict(out_format=RGBA))):
            assert _call(lib, [b"not a png"] * 2, _desc(**kw), alpha, filt) == (BAD_ARG, [0xABCD] * 2)


def test_the_existing_checks_come_first_and_unchanged(lib):
    filters = (None, _filter(F.BILINEAR), _filter(F.BICUBIC), _filter(F.NEAREST), _filter(9))
    for kw, want in ((dict(out_format=4), BAD_FORMAT), (dict(out_format=0x20), BAD_FORMAT), (dict(out_layout=2), BAD_FORMAT),
                     (dict(dtype=4), BAD_ARG), (dict(resize_flags=2), BAD_ARG), (dict(out_w=0), BAD_ARG), (dict(out_h=16385), BAD_ARG)):
        for filt in filters:
            for alpha in (None, _alpha(A.OVER), _alpha(3)):
                assert _call(lib, [b"not a png"], _desc(**kw), alpha, filt) == (want, [0xABCD]), (kw, alpha, filt)
    for filt in filters:
        # alpha's checks come before the filter's (the return value is the same; status stays unwritten)
        assert _call(lib, [b"not a png"], _desc(out_format=RGBA), _alpha(A.OVER), filt) == (BAD_ARG, [0xABCD])
        assert _call(lib, [b"not a png"], _desc(), _alpha(A.OVER, (256, 0, 0, 0)), filt) == (BAD_ARG, [0xABCD])
        assert _call(lib, [b"not a png"], None, None, filt) == (BAD_ARG, [0xABCD])
        assert _call(lib, [b"not a png"], _desc(), None, filt, out=None) == (BAD_ARG, [0xABCD])
        assert _call(lib, [b"not a png"], _desc(), None, filt, out=DUMMY + 8) == (BAD_ARG, [0xABCD])
    assert lib.debig_png_decode_batch_tensor_filter(None, None, None, None, None, None, 0, 0, None, None, None) == 0  # n == 0


def test_the_old_calls_still_refuse_resize_flags_2(lib):
    n = 1
    buf = C.create_string_buffer(b"not a png", 9)
    ins, sizes = (C.c_void_p * n)(C.addressof(buf)), (C.c_uint64 * n)(9)
    for flags in (2, 3, 0x80000000):
        d = _desc(resize_flags=flags)
        st = (C.c_uint32 * n)(0xABCD)
        assert lib.debig_png_decode_batch_tensor(ins, sizes, DUMMY, None, st, None, n, 0, C.byref(d)) == BAD_ARG
        assert lib.debig_png_decode_batch_tensor_alpha(ins, sizes, DUMMY, None, st, None, n, 0, C.byref(d), None) == BAD_ARG
        assert list(st) == [0xABCD]


def test_accepted_descriptors_reach_the_files(lib):
    """filter == NULL, every filter with every alpha mode: the files are looked at (both are broken before IHDR ends, so no
    device work follows); NULL and BILINEAR are the old call"""
    rng = np.random.default_rng(1)
    png = R.encode(R.random_image(rng, 40, 30, 6, 8), 6, 8)
    files = [b"not a png", png[:30]]
    want = (0, [R.E_SIGNATURE, R.E_CHUNK])
    for filt in (None, _filter(F.BILINEAR), _filter(F.BICUBIC), _filter(F.NEAREST)):
        for fmt in (RGBA, RGB, GRAY, RGB | 0x10):
            assert _call(lib, files, _desc(out_format=fmt), None, filt) == want
            assert _call(lib, files, _desc(out_format=fmt), _alpha(A.STRAIGHT), filt) == want
        assert _call(lib, files, _desc(out_format=RGB), _alpha(A.OVER, (255, 255, 255, 0)), filt) == want
        assert _call(lib, files, _desc(out_format=GRAY | 0x10), _alpha(A.OVER, (65535, 0, 0, 0)), filt) == want
        assert _call(lib, files, _desc(out_format=RGBA), _alpha(A.PREMULTIPLIED), filt) == want


def test_box_edges_at_32_and_64_times_the_output(lib):
    """E_BOX is decided as soon as IHDR has been read: a file cut off after IHDR gives E_BOX or the walk's E_CHUNK, no device work.
    BICUBIC antialiased: 32 L passes, 32 L + 1 is E_BOX; BILINEAR keeps 64 L / 64 L + 1; NEAREST has no scale rule; without
    antialias none has"""
    rng = np.random.default_rng(2)
    png = R.encode(R.random_image(rng, 300, 200, 2, 8), 2, 8)[:60]  # 300 x 200, IHDR intact
    ok = R.E_CHUNK
    for aa in (1, 0):
        d = _desc(out_w=2, out_h=3, resize_flags=aa)  # 32 L: 64 x 96; 64 L: 128 x 192
        boxes = [(0, 0, 64, 96), (0, 0, 65, 96), (0, 0, 64, 97), (236, 104, 64, 96), (0, 0, 128, 192), (0, 0, 129, 192), (0, 0, 128, 193),
                 (0, 0, 300, 200), (0, 0, 0, 0), (0, 0, 301, 1), (0, 0, 5, 0)]
        box_err = [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
        scale32 = [0, 1, 1, 0, 1, 1, 1, 1, 1, 0, 0]
        scale64 = [0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0]
        for filt, scale in ((F.BICUBIC, scale32), (F.BILINEAR, scale64), (None, scale64), (F.NEAREST, [0] * 11)):
            want = [Z.E_BOX if b or (aa and s) else ok for b, s in zip(box_err, scale)]
            rc, st = _call(lib, [png] * len(boxes), d, None, _filter(filt) if filt is not None else None, boxes=boxes)
            assert rc == 0 and st == want, (aa, filt, st, want)
            for b, s in zip(boxes, st):
                assert F.box_ok(filt or 0, b, 300, 200, (3, 2), aa) == (s != Z.E_BOX), (aa, filt, b)


def test_python_arguments():
    from debigulator_amd import api

    assert api.png_filter_desc() is None and api.png_filter_desc("bilinear") is None
    d = api.png_filter_desc("bicubic")
    assert (d.filter, d.reserved) == (F.BICUBIC, 0)
    d = api.png_filter_desc("nearest")
    assert (d.filter, d.reserved) == (F.NEAREST, 0)
    assert C.sizeof(api.PngFilterDesc) == C.sizeof(FilterDesc) == 8 and api.PNG_FILTERS == F.FILTERS
    for bad in ("lanczos", "cubic", 1, None):
        with pytest.raises(ValueError):
            api.png_filter_desc(bad)
    with pytest.raises(ValueError):  # (raised before the library or a device is touched)
        api.png_decode_batch_tensor([b"not a png"], (8, 8), filter="box")
    import inspect

    sig = inspect.signature(api.png_decode_batch_tensor).parameters
    assert sig["filter"].default == "bilinear" and list(sig)[-1] == "filter"


def test_symbols_are_exported(lib):
    from debigulator_amd import _native as N

    out = os.popen(f"nm -D --defined-only {N.LIB_PATH}").read()
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"debig_png_decode_batch_tensor_filter", "debig_png_resize_weights_filter", "debig_hip_png_resize_cubic_batch"} <= syms


# ---- nearest and bicubic against torch --------------------------------------------------------------------------------------

def _content(kind, h, w, Cn, P, seed):
    M = (1 << P) - 1
    dt = np.uint8 if P == 8 else np.uint16
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, M + 1, size=(h, w, Cn), dtype=np.uint16).astype(dt)
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([np.where(((x // (2 + 3 * c)) + (y // (1 + 2 * c))) % 2 == 0, M, 0) for c in range(Cn)], axis=2).astype(dt)


def test_nearest_uint_is_torch_nearest_exact():
    import torch

    for P in (8, 16):
        for (h, w), size in (((37, 53), (11, 13)), ((9, 7), (40, 61)), ((64, 48), (64, 48)), ((50, 3), (7, 100)), ((1, 1), (5, 4)),
                             ((300, 200), (1, 1)), ((23, 41), (224, 224))):
            px = _content("noise", h, w, 3, P, h + w)
            got = F.resize(px, size, "nearest", "uint", aa=bool(h % 2))
            t = torch.from_numpy(px.astype(np.float64)).permute(2, 0, 1)[None]
            want = torch.nn.functional.interpolate(t, size=size, mode="nearest-exact")[0].permute(1, 2, 0).numpy()
            assert np.array_equal(got.astype(np.float64), want), (P, h, w, size)
    px = _content("noise", 40, 30, 4, 8, 5)
    got = F.resize(px, (9, 8), "nearest", "uint", box=(3, 4, 20, 31), layout="chw")
    assert np.array_equal(got, np.transpose(F.resize(px[4:35, 3:23], (9, 8), "nearest", "uint"), (2, 0, 1)))


def _keys(x):
    x = np.abs(x)
    return np.where(x <= 1, (1.5 * x - 2.5) * x * x + 1, np.where(x < 2, ((-0.5 * x + 2.5) * x - 4) * x + 2, 0.0))


def _keys_axis(cl, L, aa):
    """float64 statement of the filter: the Keys kernel (a = -1/2) as wide as the scale when it shrinks with antialias, taps
    clipped to the crop and renormalised -> (L, cl) matrix"""
    s = max(cl / L, 1.0) if aa else 1.0
    j = np.arange(cl)[None, :] + 0.5
    c = (np.arange(L)[:, None] + 0.5) * cl / L
    k = _keys((j - c) / s)
    return k / k.sum(axis=1, keepdims=True)


def _torch_bicubic(px, size):
    import torch

    M = float((1 << (8 * px.dtype.itemsize)) - 1)
    t = torch.from_numpy(px.astype(np.float64)).permute(2, 0, 1)[None]
    o = torch.nn.functional.interpolate(t, size=size, mode="bicubic", align_corners=False, antialias=True)
    return o[0].permute(1, 2, 0).numpy().clip(0.0, M)


CASES = [  # (h, w), (H, W): shrinking, enlarging, mixed
    ((64, 48), (17, 23)), ((100, 37), (37, 30)), ((224, 300), (64, 64)), ((90, 60), (7, 5)),
    ((13, 17), (40, 61)), ((30, 20), (224, 224)), ((5, 3), (9, 16)),
    ((40, 90), (90, 40)), ((77, 20), (20, 77)), ((50, 50), (50, 20)),
]


@pytest.mark.parametrize("P", [8, 16])
def test_bicubic_is_close_to_torch_float64(P):
    """UINT and float32 outputs of the restatement against interpolate(mode="bicubic", align_corners=False, antialias=True) in
    float64, clamped to [0, M]; without antialias torch's a = -0.75 border-replicating variant is NOT the reference: an
    enlargement is compared with antialias=True (the two rules coincide), a shrinking or mixed one with the float64 Keys
    statement above.  Bounds: twice the maxima measured on these cases (module docstring)."""
    M = (1 << P) - 1
    worst_f, worst_u = 0.0, 0.0
    for k, ((h, w), size) in enumerate(CASES):
        for kind in ("noise", "edges"):
            px = _content(kind, h, w, 3, P, k)
            want_aa = _torch_bicubic(px, size)
            ky, kx = _keys_axis(h, size[0], True), _keys_axis(w, size[1], True)
            keys_aa = np.einsum("Yy,yxc,Xx->YXc", ky, px.astype(np.float64), kx).clip(0, M)
            assert np.abs(keys_aa - want_aa).max() < 1e-6 * M  # the float64 statement IS torch's antialiased bicubic
            for aa in (True, False):
                if aa or (size[0] >= h and size[1] >= w):
                    want = want_aa
                else:
                    ky, kx = _keys_axis(h, size[0], False), _keys_axis(w, size[1], False)
                    want = np.einsum("Yy,yxc,Xx->YXc", ky, px.astype(np.float64), kx).clip(0, M)
                f = F.resize(px, size, "bicubic", "float32", aa, scale=(M, M, M, M)).astype(np.float64)
                u = F.resize(px, size, "bicubic", "uint", aa).astype(np.float64)
                ef, eu = float(np.abs(f - want).max()), float(np.abs(u - np.rint(want)).max())
                worst_f, worst_u = max(worst_f, ef), max(worst_u, eu)
                assert ef <= BOUNDS[P][0] and eu <= BOUNDS[P][1], ((h, w), size, kind, aa, ef, eu)
    print(f"P {P}: max |float32 output - torch float64| {worst_f:.4f} levels (bound {BOUNDS[P][0]}), UINT {worst_u:.0f} levels (bound {BOUNDS[P][1]})")


def test_alpha_identities_of_the_restatement():
    rng = np.random.default_rng(3)
    for P in (8, 16):
        M = (1 << P) - 1
        for Cn in (2, 4):
            px = _content("edges", 31, 50, Cn, P, 0)
            px[:, :, -1] = rng.integers(0, M + 1, size=(31, 50))
            opaque, clear = px.copy(), px.copy()
            opaque[:, :, -1], clear[:, :, -1] = M, 0
            for filt in ("bicubic", "nearest"):
                for aa in (True, False):
                    for size in ((13, 17), (31, 50), (60, 77)):
                        bg = [1, M // 2, M - 1]
                        v, _ = F.resize_alpha_int(opaque, size, filt, A.OVER, aa, None, bg)
                        assert np.array_equal(v, F.resize_int(opaque[:, :, :-1], size, filt, aa)[0])
                        v, _ = F.resize_alpha_int(clear, size, filt, A.OVER, aa, None, bg)
                        assert (v == (np.array(bg[:Cn - 1], np.int64) << (30 - P))).all()
                        v, _ = F.resize_alpha_int(opaque, size, filt, A.PREMULTIPLIED, aa)
                        assert np.array_equal(v, F.resize_int(opaque, size, filt, aa)[0])
                        v, _ = F.resize_alpha_int(px, size, filt, A.PREMULTIPLIED, aa)
                        assert (v[:, :, :-1] <= v[:, :, -1:]).all() and v.min() >= 0 and v.max() <= M << (30 - P)
