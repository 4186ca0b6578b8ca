"""APNG without a GPU: the reference of tests/apng_ref.py against PIL (binary alpha, every dispose / blend pair,
sub-regions, default image in or out), the integer OVER rule against the real-number one, and the animation rules of
include/decode_png.h in debig_apng_info_get (host only) and in the reference, one file per rule."""
import ctypes as C
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import apng_ref as A  # noqa: E402
import png_spec_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------------ vs PIL
def pil_files(dispose, blend, default_image, seed=0):
    """an RGBA animation written by PIL (binary alpha: a moving opaque rectangle with holes on a transparent canvas,
    so PIL crops the later frames to sub-regions) -> (file, [PIL's composited frames, the default image dropped])"""
    from PIL import Image

    rng = np.random.default_rng(seed)
    W, H = 29, 21
    ims = []
    for k in range(5):
        a = np.zeros((H, W, 4), np.uint8)
        x, y = 2 + 3 * k, 1 + 2 * k
        rect = rng.integers(0, 256, size=(7, 9, 4), dtype=np.uint8)
        rect[..., 3] = np.where(rng.random((7, 9)) < 0.2, 0, 255)
        rect[rect[..., 3] == 0] = 0
        a[y: y + 7, x: x + 9] = rect
        ims.append(Image.fromarray(a, "RGBA"))
    if default_image:
        # PIL renders the first animation frame over the default image, where the APNG specification starts from a
        # transparent black canvas: a transparent black default image makes the two agree
        ims[0] = Image.fromarray(np.zeros((H, W, 4), np.uint8), "RGBA")
    buf = io.BytesIO()
    ims[0].save(buf, "PNG", save_all=True, append_images=ims[1:], disposal=dispose, blend=blend,
                default_image=default_image)
    data = buf.getvalue()
    im = Image.open(io.BytesIO(data))
    frames = []
    for k in range(im.n_frames):
        im.seek(k)
        frames.append(np.asarray(im.convert("RGBA")))
    if default_image:
        frames = frames[1:]
    return data, np.stack(frames)


@pytest.mark.parametrize("default_image", [False, True])
@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("dispose", [0, 1, 2])
def test_reference_against_pil(dispose, blend, default_image):
    pytest.importorskip("PIL.Image")
    data, expect = pil_files(dispose, blend, default_image, seed=dispose * 4 + blend * 2 + default_image)
    st, got, info = A.decode(data)
    assert st == R.OK
    assert info["default_is_frame"] == int(not default_image)
    assert any(f["width"] < info["width"] or f["height"] < info["height"] for f in info["frames"]), "no sub-region"
    assert got.shape == expect.shape
    assert np.array_equal(got, expect), np.argwhere(got != expect)[:4]


def test_integer_over_against_the_real_formula():
    """u = sa 255, v = (255 - sa) da, al = u + v, c = (sc u + dc v) / al, a = al / 255, truncating, against the APNG
    specification's real-number blend: within 1 per channel over 10^6 random (sc, sa, dc, da)"""
    rng = np.random.default_rng(7)
    n = 1_000_000
    s = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    d = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    s[: n // 100, 3] = 0
    s[n // 100: n // 50, 3] = 255
    got = A.over(s, d).astype(np.float64)
    sa, da = s[:, 3:4] / 255.0, d[:, 3:4] / 255.0
    ao = sa + (1 - sa) * da
    with np.errstate(invalid="ignore", divide="ignore"):
        co = (s[:, :3] * sa + d[:, :3] * da * (1 - sa)) / ao
    co = np.where(ao > 0, co, d[:, :3])
    exp = np.concatenate([co, ao * 255.0], axis=1)
    assert np.abs(got - exp).max() <= 1.0 + 1e-9
    assert np.array_equal(A.over(s[: n // 100], d[: n // 100]), d[: n // 100])
    assert np.array_equal(A.over(s[n // 100: n // 50], d[n // 100: n // 50]), s[n // 100: n // 50])


# ------------------------------------------------------------------------------------------------ animation rules
def _base_chunks():
    """a good APNG: 8 x 6 RGBA, the IDAT image is frame 0, two sub-region frames of two fdAT chunks each
    -> [IHDR, acTL, fcTL0, IDAT, fcTL1, fdAT2, fdAT3, fcTL4, fdAT5, fdAT6, IEND]"""
    rng = np.random.default_rng(3)
    fr = [A.frame(R.random_image(rng, 8, 6, 6, 8)),
          A.frame(R.random_image(rng, 3, 2, 6, 8), x=4, y=3, dispose=A.PREVIOUS, blend=A.OVER),
          A.frame(R.random_image(rng, 4, 4, 6, 8), x=0, y=2, dispose=A.BACKGROUND)]
    return A.apng_chunks(fr, 6, 8, fdat_split=[9])


def _fctl_with(body, **kw):
    names = ["seq", "width", "height", "x", "y", "dn", "dd", "dispose", "blend"]
    v = dict(zip(names, struct.unpack(">IIIIIHHBB", body)))
    v.update(kw)
    return struct.pack(">IIIIIHHBB", *[v[k] for k in names])


def _set(ch, i, body):
    ch = list(ch)
    ch[i] = (ch[i][0], body)
    return ch


def anim_cases():
    """(name, file) pairs, each breaking exactly one animation rule of include/decode_png.h"""
    B = _base_chunks()
    assert [t for t, _ in B] == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fdAT", b"fcTL", b"fdAT", b"fdAT",
                                 b"IEND"]
    W, H = 8, 6
    c = []
    c.append(("acTL after IDAT", B[:1] + B[2:4] + [B[1]] + B[4:]))
    c.append(("acTL twice", B[:2] + [B[1]] + B[2:]))
    c.append(("acTL length", _set(B, 1, B[1][1] + b"\0")))
    c.append(("acTL zero frames", _set(B, 1, struct.pack(">II", 0, 0))))
    c.append(("fcTL length", _set(B, 4, B[4][1] + b"\0")))
    c.append(("fcTL width 0", _set(B, 4, _fctl_with(B[4][1], width=0))))
    c.append(("fcTL height 0", _set(B, 4, _fctl_with(B[4][1], height=0))))
    c.append(("fcTL x_off + width > W", _set(B, 4, _fctl_with(B[4][1], x=W - 3 + 1))))
    c.append(("fcTL y_off + height > H", _set(B, 4, _fctl_with(B[4][1], y=H - 2 + 1))))
    c.append(("fcTL x_off wraps 32 bits", _set(B, 4, _fctl_with(B[4][1], x=0xFFFFFFFF))))
    c.append(("fcTL y_off wraps 32 bits", _set(B, 4, _fctl_with(B[4][1], y=0xFFFFFFFE))))
    c.append(("dispose_op 3", _set(B, 4, _fctl_with(B[4][1], dispose=3))))
    c.append(("blend_op 2", _set(B, 4, _fctl_with(B[4][1], blend=2))))
    two = A.renumber(B[:2] + [B[2], B[2]] + B[3:])
    two = _set(two, 1, struct.pack(">II", 4, 0))
    c.append(("two fcTL before IDAT", two))
    c.append(("fcTL before IDAT not at (0, 0)", _set(B, 2, _fctl_with(B[2][1], x=1, width=W - 1))))
    c.append(("fcTL before IDAT not the whole canvas", _set(B, 2, _fctl_with(B[2][1], height=H - 1))))
    c.append(("fdAT before IDAT", A.renumber(B[:3] + [A.fdat(0, B[3][1])] + B[3:])))
    c.append(("fdAT shorter than 4", B[:6] + [(b"fdAT", b"\0\0\3")] + B[7:]))
    c.append(("fdAT right after IDAT", A.renumber(B[:4] + [A.fdat(0, b"\0")] + B[4:])))
    c.append(("frame without fdAT (middle)", A.renumber(B[:5] + B[7:])))
    c.append(("frame without fdAT (last)", A.renumber(B[:8] + B[10:])))
    c.append(("sequence number skipped", B[:5] + [A.fdat(3, B[5][1][4:])] + B[6:]))
    c.append(("sequence starts at 1", [(t, struct.pack(">I", struct.unpack(">I", d[:4])[0] + 1) + d[4:])
                                       if t in (b"fcTL", b"fdAT") else (t, d) for t, d in B]))
    c.append(("acTL claims more frames", _set(B, 1, struct.pack(">II", 4, 0))))
    c.append(("acTL claims fewer frames", _set(B, 1, struct.pack(">II", 2, 0))))
    # the default image is not a frame: an fdAT before any fcTL after the IDAT
    c.append(("no fcTL since the IDAT", A.renumber(B[:2] + [B[3], A.fdat(0, B[5][1][4:])] + B[4:])))
    return [(name, A.assemble(ch)) for name, ch in c]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    from debigulator_amd import api

    return api


def test_base_file_is_good(lib):
    data = A.assemble(_base_chunks())
    st, px, info = A.decode(data)
    assert st == R.OK and px.shape == (3, 6, 8, 4)
    st2, info2 = lib.apng_info(data)
    assert st2 == 0 and info2 == info
    assert info["frames"][1] == dict(x=4, y=3, width=3, height=2, delay_num=1, delay_den=10, dispose=2, blend=1)


@pytest.mark.parametrize("case", range(26))
def test_every_animation_rule(lib, case):
    cases = anim_cases()
    assert len(cases) == 26
    name, data = cases[case]
    assert R.decode(data)[0] == R.OK or R._walk(data)[0] == R.OK, name  # the still-image walk passes
    assert A.decode(data)[0] == A.E_ANIM, name
    st, _ = lib.apng_info(data)
    assert st == A.E_ANIM, (name, st)
    assert lib.PNG_STATUS[st] == "animation"


def test_still_png_is_one_frame(lib):
    rng = np.random.default_rng(4)
    data = R.encode(R.random_image(rng, 9, 7, 2, 16), 2, 16, 1)
    st, info = lib.apng_info(data)
    assert st == 0
    assert (info["num_frames"], info["num_plays"], info["default_is_frame"]) == (1, 0, 1)
    assert info["frames"] == [dict(x=0, y=0, width=9, height=7, delay_num=0, delay_den=0, dispose=0, blend=0)]
    est, px, einf = A.decode(data)
    assert est == 0 and einf == info
    assert np.array_equal(px[0], R.decode(data)[1])


def test_fctl_and_fdat_without_actl_are_ignored(lib):
    B = _base_chunks()
    data = A.assemble(B[:1] + B[2:])
    st, info = lib.apng_info(data)
    assert st == 0 and info["num_frames"] == 1 and info["frames"][0]["width"] == 8
    est, px, einf = A.decode(data)
    assert est == 0 and einf == info and px.shape == (1, 6, 8, 4)
    # ... even when they would break every rule
    bad = A.assemble(B[:1] + [A.fdat(7, b"")] + B[2:])
    assert lib.apng_info(bad)[0] == 0 and A.decode(bad)[0] == 0


def test_walk_errors_come_first(lib):
    """a broken still-image rule outranks a broken animation rule"""
    B = _base_chunks()
    bad = A.assemble(B[:1] + [(b"ABCD", b"")] + B[1:2] + [B[1]] + B[2:])  # unknown critical chunk, then acTL twice
    assert A.decode(bad)[0] == R.E_CHUNK
    assert lib.apng_info(bad)[0] == R.E_CHUNK
