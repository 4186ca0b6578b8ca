"""debig_apng_decode_batch on the MI355X (include/decode_png.h): a mixed batch of every (colour type, depth), Adam7,
tRNS, 16-bit, split fdAT chunks, sub-regions, PREVIOUS on frame 0 and fractional-alpha OVER against tests/apng_ref.py
(tuned routing and forced general), PIL-written binary-alpha animations against PIL, still PNGs against
debig_png_decode_batch, every E_ANIM rule and the other error statuses beside good files, E_OUTPUT at the exact size,
and a batch of 256 files x 8 frames."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import apng_ref as A  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_apng_cpu as T  # noqa: E402
import test_gpu_png_spec as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as M

    return M


def _samples(rng, w, h, ct, depth, n_pal, key):
    s = R.random_image(rng, w, h, ct, depth, n_pal)
    if key is not None:  # make the key appear
        s[:: 3, :: 2] = np.asarray(key, dtype=s.dtype).reshape(1, 1, -1)
    return s


def _mixed_file(rng, ct, depth, il, trns, default_in, k):
    W, H = 21 + k % 5, 14 + k % 3
    pal = t = key = None
    n_pal = None
    if ct == 3:
        n_pal = int(rng.integers(2, (1 << depth) + 1))
        pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(n_pal)]
        if trns:
            t = bytes(rng.integers(0, 256, size=n_pal - 1, dtype=np.uint8))
    elif trns and ct in (0, 2):
        key = tuple(int(v) for v in rng.integers(0, 1 << depth, size=3 if ct == 2 else 1))
        t = np.asarray(key, dtype=">u2").tobytes()
    frames = [A.frame(_samples(rng, W, H, ct, depth, n_pal, key), dispose=A.PREVIOUS, blend=A.OVER)]
    regions = [(3, 2, 7, 5), (0, 0, W, H), (W - 6, H - 4, 6, 4), (1, 5, 4, 3)]
    ops = [(A.PREVIOUS, A.OVER), (A.NONE, A.OVER), (A.BACKGROUND, A.SOURCE), (A.NONE, A.OVER)]
    for (x, y, w, h), (dop, bop) in zip(regions, ops):
        frames.append(A.frame(_samples(rng, w, h, ct, depth, n_pal, key), x=x, y=y, dispose=dop, blend=bop,
                              delay=(k, 100)))
    default = None if default_in else _samples(rng, W, H, ct, depth, n_pal, key)
    mode = ("stored", "fixed", "default")[(ct + depth + il) % 3]
    return A.encode(frames, ct, depth, interlace=il, palette=pal, trns=t, default=default, num_plays=k % 3,
                    fdat_split=[5, 3] if k % 2 else None, mode=mode)


def mixed_batch():
    rng = np.random.default_rng(2025)
    files, k = [], 0
    for ct, depths in R.DEPTHS.items():
        for depth in depths:
            for il in (0, 1):
                for trns in ((0, 1) if ct in (0, 2, 3) else (0,)):
                    files.append(((ct, depth, il, trns), _mixed_file(rng, ct, depth, il, trns, k % 3 != 2, k)))
                    k += 1
    return files


def _check_against_reference(out, files):
    for (key, data), (st, px, inf) in zip(files, out):
        est, epx, einf = A.decode(data)
        assert est == R.OK, key
        assert st == 0, (key, st)
        assert inf == einf, key
        assert px.shape == epx.shape, key
        assert np.array_equal(px, epx), (key, np.argwhere(px != epx)[:4])


@pytest.mark.parametrize("force_general", [False, True])
def test_mixed_batch_matches_reference(api, force_general):
    files = mixed_batch()
    # frames the still-image path cannot produce: sub-regions under OVER and PREVIOUS, fractional alpha
    infos = [A.decode(d)[2] for _, d in files]
    assert any(f["width"] < i["width"] and f["blend"] == A.OVER for i in infos for f in i["frames"])
    assert any(f["dispose"] == A.PREVIOUS and k > 0 for i in infos for k, f in enumerate(i["frames"]))
    assert any(i["frames"][0]["dispose"] == A.PREVIOUS for i in infos)
    assert any(i["default_is_frame"] == 0 for i in infos)
    frac = [px for _, px, _ in (A.decode(d) for (ct, _, _, _), d in files if ct in (4, 6))]
    assert any(((p[..., 3] > 0) & (p[..., 3] < 255)).any() for p in frac)
    _check_against_reference(api.apng_decode_batch([d for _, d in files], force_general=force_general), files)


def test_pil_files_match_pil(api):
    pytest.importorskip("PIL.Image")
    cases = [T.pil_files(d, b, di, seed=40 + d * 4 + b * 2 + di) for d in range(3) for b in range(2) for di in (0, 1)]
    out = api.apng_decode_batch([data for data, _ in cases])
    for (data, expect), (st, px, _) in zip(cases, out):
        assert st == 0
        assert np.array_equal(px, expect)


def test_still_png_equals_png_decode_batch(api):
    files = [d for _, d in G._all_formats()]
    still = api.png_decode_batch(files)
    for force_general in (False, True):
        anim = api.apng_decode_batch(files, force_general=force_general)
        for (st0, px0, _), (st1, px1, inf) in zip(still, anim):
            assert st0 == st1 == 0 and inf["num_frames"] == 1
            assert px1.shape == (1,) + px0.shape and px1[0].tobytes() == px0.tobytes()


def _good_anim(rng, k=0):
    fr = [A.frame(R.random_image(rng, 20, 11, 6, 8)),
          A.frame(R.random_image(rng, 7, 5, 6, 8), x=3, y=2, dispose=A.PREVIOUS, blend=A.OVER),
          A.frame(R.random_image(rng, 20, 11, 6, 8), blend=A.OVER),
          A.frame(R.random_image(rng, 9, 4, 6, 8), x=11, y=7, dispose=A.BACKGROUND)]
    return fr


def error_files():
    rng = np.random.default_rng(9)
    fr = _good_anim(rng)
    good = A.encode(fr, 6, 8, fdat_split=[6])
    z3 = R.zlib_stream(R.scanlines(fr[3]["samples"], 6, 8), "stored")
    z1 = zlib.compress(R.scanlines(fr[1]["samples"], 6, 8))
    cases = [(name, data, A.E_ANIM) for name, data in T.anim_cases()]
    crc = bytearray(good)
    at = bytes(good).rindex(b"fdAT")
    crc[at + 4 + 4 + 10] ^= 0x40  # a DEFLATE byte of the last fdAT chunk: its stored CRC no longer matches
    cases += [("crc in fdAT", bytes(crc), R.E_CRC),
              ("frame 3 inflate", A.encode(fr, 6, 8, zdata={3: z3[:2] + bytes([0x01, 5, 0, 0, 0]) + z3[7:]}), R.E_INFLATE),
              ("frame 1 adler", A.encode(fr, 6, 8, zdata={1: z1[:-4] + bytes(4)}), R.E_ADLER),
              ("frame 2 zlib", A.encode(fr, 6, 8, zdata={2: b"\x78"}), R.E_ZLIB),
              ("frame 2 short", A.encode(fr, 6, 8, zdata={2: zlib.compress(R.scanlines(fr[2]["samples"], 6, 8)[:-3])}),
               R.E_DATA_SHORT),
              ("frame 1 filter", A.encode([fr[0], A.frame(fr[1]["samples"], x=3, y=2)] + fr[2:], 6, 8,
                                          zdata={1: zlib.compress(b"\x07" + R.scanlines(fr[1]["samples"], 6, 8)[1:])}),
               R.E_FILTER)]
    for name, data, st in cases:
        assert A.decode(data)[0] == st, name
    return good, cases


def test_every_error_beside_good_files(api):
    good, cases = error_files()
    goods = [d for _, d in mixed_batch()[::4]] + [good]
    batch, expect = [], []
    for k, (name, data, st) in enumerate(cases):
        batch += [data, goods[k % len(goods)]]
        expect += [(name, st), ("good", 0)]
    for force_general in (False, True):
        out = api.apng_decode_batch(batch, force_general=force_general)
        for data, (name, st), (got, px, _) in zip(batch, expect, out):
            assert got == st, (name, got)
            if st == 0:
                assert np.array_equal(px, A.decode(data)[1]), name


def test_output_cap_exact(api):
    rng = np.random.default_rng(10)
    datas = [A.encode(_good_anim(rng), 6, 8), A.encode(_good_anim(rng), 6, 8)]
    L = api._apng_lib()
    size = 4 * 20 * 11 * 4
    outs = [np.zeros(size, np.uint8) for _ in datas]
    ins = [np.frombuffer(d, np.uint8) for d in datas]
    st = (C.c_uint32 * 2)()
    rc = L.debig_apng_decode_batch((C.c_void_p * 2)(*[a.ctypes.data for a in ins]), (C.c_uint64 * 2)(*[len(d) for d in datas]),
                                   (C.c_void_p * 2)(*[o.ctypes.data for o in outs]), (C.c_uint64 * 2)(size - 1, size),
                                   st, None, 2, 0)
    from debigulator_amd import _native as N

    N.check(rc, "debig_apng_decode_batch")
    assert list(st) == [R.E_OUTPUT, 0]
    assert np.array_equal(outs[1].reshape(4, 11, 20, 4), A.decode(datas[1])[1])


def test_large_batch(api):
    """256 files x 8 frames: every launch carries thousands of frames"""
    rng = np.random.default_rng(11)
    distinct = []
    for k in range(16):
        ct = (6, 2, 0, 3)[k % 4]
        pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(16)] if ct == 3 else None
        W, H = 48 + k, 24 + k % 5
        fr = [A.frame(R.random_image(rng, W, H, ct, 8, 16))]
        for j in range(7):
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            fr.append(A.frame(R.random_image(rng, w, h, ct, 8, 16), x=int(rng.integers(0, W - w + 1)),
                              y=int(rng.integers(0, H - h + 1)), dispose=j % 3, blend=(j // 3) % 2))
        distinct.append(A.encode(fr, ct, 8, palette=pal, fdat_split=[4] if k % 2 else None))
    files = [distinct[k % 16] for k in range(256)]
    refs = [A.decode(d) for d in distinct]
    out = api.apng_decode_batch(files)
    for k, (st, px, inf) in enumerate(out):
        est, epx, einf = refs[k % 16]
        assert st == est == 0 and inf == einf
        assert px.shape[0] == 8 and np.array_equal(px, epx), k
