"""debig_png_decode_batch_dev / debig_png_decode_batch_layout on the MI355X (include/decode_png.h): pixels that stay on the
device, interleaved or channel-planar, against the numpy converter of tests/png_out_format_ref.py and against the merged
host path; the re-routing of tuned-route files to the planar kernel; untouched gaps, E_OUTPUT and failing files in a raw
arena; every error status; a 4096 x 4096 16-bit image; the tensors' device and storage."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_out_format_ref as F  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_gpu_png_spec as G  # noqa: E402

pytestmark = pytest.mark.gpu
MODE_DEPTHS = [(F.MODES[f & 15], F.DEPTHS[f & 0x30]) for f in F.FORMATS]
LAYOUTS = ["hwc", "chw"]


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A

    return A


@pytest.fixture(scope="module")
def datas():
    return [d for _, d in G._all_formats()]


def _np(t):
    """a result tensor on the host, 16-bit results as uint16 whatever dtype the installed torch gave them"""
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


_REF = {}


def _want(data, fmt, layout):
    if (data, fmt) not in _REF:
        _REF[(data, fmt)] = F.decode(data, fmt)
    st, px, inf = _REF[(data, fmt)]
    assert st == R.OK
    return (np.transpose(px, (2, 0, 1)) if layout == "chw" else px), inf


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode,depth", MODE_DEPTHS)
def test_device_output_every_format_and_layout(api, datas, mode, depth, layout):
    fmt = api.png_out_format(mode, depth)
    host = api.png_decode_batch(datas, mode=mode, depth=depth)
    for general in (False, True):
        out = api.png_decode_batch_device(datas, mode=mode, depth=depth, layout=layout, force_general=general)
        assert len(out) == len(datas)
        for data, (st, t, inf), (hst, hpx, _) in zip(datas, out, host):
            want, einf = _want(data, fmt, layout)
            assert st == 0 and hst == 0, (einf, hex(fmt), layout, st)
            assert inf == einf
            got = _np(t)
            assert got.dtype == want.dtype and got.shape == want.shape, (einf, hex(fmt), layout)
            assert np.array_equal(got, want), (einf, hex(fmt), layout, np.argwhere(got != want)[:4])
            if layout == "hwc":  # the merged host path, byte for byte
                assert got.tobytes() == hpx.tobytes(), (einf, hex(fmt))


@pytest.mark.parametrize("mode,depth", MODE_DEPTHS)
def test_host_chw_is_the_transposed_hwc(api, datas, mode, depth):
    a = api.png_decode_batch(datas, mode=mode, depth=depth)
    for general in (False, True):
        b = api.png_decode_batch(datas, mode=mode, depth=depth, layout="chw", force_general=general)
        for (sa, pa, ia), (sb, pb, ib) in zip(a, b):
            assert sa == sb == 0 and ia == ib
            assert pb.dtype == pa.dtype and pb.shape == (pa.shape[2], pa.shape[0], pa.shape[1])
            assert np.array_equal(pb, np.transpose(pa, (2, 0, 1))), ia


@pytest.mark.parametrize("mode,depth", [("rgba", 8), ("rgb", 8), ("native", "native"), ("rgba", 16), ("gray_alpha", 8)])
def test_tuned_route_files_in_chw(api, mode, depth):
    """non-interlaced RGB8 / RGBA8 files take the tuned kernels for interleaved RGBA8; in CHW they go to the planar kernel"""
    rng = np.random.default_rng(31)
    datas = [R.encode(R.random_image(rng, w, 37, ct, 8), ct, 8) for ct in (2, 6) for w in (1, 64, 333)]
    fmt = api.png_out_format(mode, depth)
    dev = api.png_decode_batch_device(datas, mode=mode, depth=depth, layout="chw")
    host = api.png_decode_batch(datas, mode=mode, depth=depth, layout="chw")
    for data, (st, t, _), (hst, hpx, _) in zip(datas, dev, host):
        want, einf = _want(data, fmt, "chw")
        assert st == 0 and hst == 0
        assert np.array_equal(_np(t), want) and np.array_equal(hpx, want), einf
        assert _np(t).dtype == want.dtype == hpx.dtype


def _raw_dev(api, datas, fmt, layout, gaps, caps=None, flags=0):
    """debig_png_decode_batch_dev on an arena pre-filled with 0xA5, exact caps unless given, gaps[i] bytes after region i
    -> (statuses, arena bytes as numpy, offsets, exact sizes)"""
    import torch
    from debigulator_amd import _native as N

    L = api._png_spec_lib()
    n = len(datas)
    exact = []
    for d in datas:
        st, inf = api.png_info(d)
        exact.append(api.png_out_layout(inf, F.MODES[fmt & 15], F.DEPTHS[fmt & 0x30])[2] if st == 0 else 0)
    caps = list(exact) if caps is None else caps
    offs, total = [], 0
    for i in range(n):
        offs.append(total)
        total += (exact[i] + 15) // 16 * 16 + gaps[i % len(gaps)]
    arena = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ins = [np.frombuffer(d, np.uint8) for d in datas]
    st = (C.c_uint32 * n)()
    rc = L.debig_png_decode_batch_dev((C.c_void_p * n)(*[a.ctypes.data for a in ins]), (C.c_uint64 * n)(*[len(d) for d in datas]),
                                      arena.data_ptr(), (C.c_uint64 * n)(*offs), (C.c_uint64 * n)(*caps), st, None, n, flags,
                                      fmt, api.png_layout_code(layout))
    N.check(rc, "debig_png_decode_batch_dev")
    return list(st), arena.cpu().numpy(), offs, exact


def _assert_outside_untouched(a, offs, sizes, written):
    mask = np.ones(len(a), dtype=bool)
    for o, s, w in zip(offs, sizes, written):
        if w:
            mask[o: o + s] = False
    assert (a[mask] == 0xA5).all(), "bytes outside the images' own regions were written"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", [F.RGBA, F.RGB, F.GRAY_ALPHA | F.D16, F.NATIVE | F.D_NATIVE, F.RGBA | F.D16])
def test_raw_arena_gaps_caps_and_failing_files(api, datas, fmt, layout):
    rng = np.random.default_rng(41)
    tuned = [R.encode(R.random_image(rng, w, 23, ct, 8), ct, 8) for ct in (2, 6) for w in (5, 333)]
    good = datas[::4] + tuned
    crc = bytearray(good[1])
    crc[len(crc) // 2] ^= 0x20
    files = good[:3] + [bytes(crc)] + good[3:5] + [good[2][: len(good[2]) * 2 // 3]] + good[5:]
    bad = {3: R.E_CRC, 6: R.E_CHUNK}  # the truncated file: a chunk that runs past the end of the file
    gaps = [16, 4096, 48, 1024, 32, 256]
    for flags in (0, api.PNG_FORCE_GENERAL):
        st, a, offs, exact = _raw_dev(api, files, fmt, layout, gaps, flags=flags)
        for i, d in enumerate(files):
            if i in bad:
                assert st[i] == bad[i], (i, st[i])
                continue
            want, einf = _want(d, fmt, layout)
            assert st[i] == 0, (einf, st[i])
            assert a[offs[i]: offs[i] + exact[i]].tobytes() == np.ascontiguousarray(want).tobytes(), (einf, hex(fmt), layout)
        _assert_outside_untouched(a, offs, exact, [i not in bad for i in range(len(files))])
    # a cap one byte short: E_OUTPUT and an untouched region, the neighbours correct
    for victim in (0, 4, len(files) - 1):
        caps = list(exact)
        caps[victim] -= 1
        st, a, offs, exact = _raw_dev(api, files, fmt, layout, gaps, caps=caps)
        assert st[victim] == R.E_OUTPUT
        for i, d in enumerate(files):
            if i in bad or i == victim:
                continue
            assert st[i] == 0
            assert a[offs[i]: offs[i] + exact[i]].tobytes() == np.ascontiguousarray(_want(d, fmt, layout)[0]).tobytes()
        _assert_outside_untouched(a, offs, exact, [i not in bad and i != victim for i in range(len(files))])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_error_status(api, layout):
    cases = G._error_files()
    fs = G._all_formats()[::3]
    batch, expect = [], []
    for k, (name, data, st) in enumerate(cases):
        batch += [data, fs[k % len(fs)][1]]
        expect += [(name, st), ("good", 0)]
    for mode, depth in (("rgba", 8), ("rgb", 16), ("native", "native")):
        fmt = api.png_out_format(mode, depth)
        out = api.png_decode_batch_device(batch, mode=mode, depth=depth, layout=layout)
        for data, (name, st), (got, t, _) in zip(batch, expect, out):
            assert got == st, (name, got, layout)
            if st == 0:
                assert np.array_equal(_np(t), _want(data, fmt, layout)[0])
            else:
                assert t is None
    for name, data, st in cases:
        assert api.png_decode_batch_device([data], layout=layout)[0][0] == st, name
        assert api.png_decode_batch_device([data], layout=layout, force_general=True)[0][0] == st, name
    # files that fail in the de-filter write only inside their own region
    defilter = [d for _, d, st in cases if st in (R.E_FILTER, R.E_PALETTE)]
    st, a, offs, exact = _raw_dev(api, defilter, F.RGBA, layout, [64])
    assert all(s in (R.E_FILTER, R.E_PALETTE) for s in st)
    _assert_outside_untouched(a, offs, exact, [True] * len(defilter))


def test_big_16_bit_image_to_chw_planes(api):
    """4096 x 4096 16-bit RGBA, every row filter type 0 (scanlines made here, so the expected pixels are the samples)"""
    import torch

    rng = np.random.default_rng(9)
    s = rng.integers(0, 65536, size=(4096, 4096, 4), dtype=np.uint16)
    rows = np.zeros((4096, 1 + 4096 * 8), np.uint8)
    rows[:, 1:] = s.astype(">u2").reshape(4096, -1).view(np.uint8)
    big = R.encode(s[:1, :1], 6, 16, zdata=zlib.compress(rows.tobytes(), 1),
                   ihdr=np.array([4096, 4096], ">u4").tobytes() + bytes([16, 6, 0, 0, 0]))
    del rows
    st, t, inf = api.png_decode_batch_device([big], mode="rgba", depth=16, layout="chw")[0]
    assert st == 0 and tuple(t.shape) == (4, 4096, 4096)
    assert t.dtype == getattr(torch, "uint16", torch.int16)
    got = _np(t)
    for c in range(4):
        assert np.array_equal(got[c], s[:, :, c]), c
    st, t, _ = api.png_decode_batch_device([big], mode="rgb", depth=8, layout="chw")[0]
    assert st == 0 and np.array_equal(_np(t)[1], (s[:, :, 1] >> 8).astype(np.uint8))


def test_tensors_are_views_of_one_arena_on_the_device(api, datas, gpu_device):
    import torch

    for layout in LAYOUTS:
        out = api.png_decode_batch_device(datas[:6], mode="native", depth="native", layout=layout, device=gpu_device)
        ts = [t for _, t, _ in out]
        assert all(t.device == torch.device(gpu_device) for t in ts)
        assert len({t.untyped_storage().data_ptr() for t in ts}) == 1
        assert all(t.data_ptr() % 16 == 0 for t in ts)
        for (st, t, inf), d in zip(out, datas):
            ch, bs, _ = api.png_out_layout(inf, "native", "native")
            assert tuple(t.shape) == ((ch, inf["height"], inf["width"]) if layout == "chw" else (inf["height"], inf["width"], ch))
            assert t.element_size() == bs
