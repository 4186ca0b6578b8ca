"""debig_png_decode_batch_color_labels_warp on the MI355X (include/decode_png.h; api.png_decode_batch_color_labels(..., warp=)):
the whole call BIT FOR BIT against the numpy restatement tests/png_color_label_warp_ref.py applied to the RGB8 pixels of
tests/png_color_label_ref.py.  One batch of six small mask files -- RGB8 (64 x 48, the largest), RGBA8, a 4-bit palette file, an
8-bit palette file with tRNS, 2-bit grey and Adam7 RGB8 --, outputs of 1 x 1, 33 x 65 and 64 x 96, random matrices from
png_warp_matrix under both borders, PACK and MAP, `unmatched` exact; the identity, the flips and the quarter turns against
numpy.flip / numpy.rot90 of the un-warped call; the grid shared with png_decode_batch_labels(warp=); per-image maps; a mixed batch
whose failed files keep `fill`."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_label_ref as CR  # noqa: E402
import png_color_label_warp_ref as CW  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_warp_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (33, 65), (64, 96)]  # (H, W)
NAN = ((1.0, 0.0, math.nan), (0.0, 1.0, 0.0))
BORDERS = {"constant": CW.CONSTANT, "clamp": CW.CLAMP}


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


_D = {}


def _blocks(rng, w, h, top):
    return np.kron(rng.integers(0, top, size=((h + 3) // 4, (w + 4) // 5)), np.ones((4, 5), dtype=np.int64))[:h, :w]


def _data():
    """files: [(data, (w, h))] -- blocky masks with a few stray pixels; pal: the palettes of the two palette files"""
    if not _D:
        rng = np.random.default_rng(2027)
        ft = lambda p, y: y % 5  # noqa: E731
        c9 = rng.integers(0, 256, size=(9, 3)).astype(np.uint8)
        pal4 = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(13)]
        pal8 = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(200)]
        files = []
        for w, h, kind in ((64, 48, "rgb"), (40, 33, "rgba"), (33, 17, "pal4"), (45, 30, "pal8"), (21, 19, "g2"), (37, 29, "rgb7")):
            if kind in ("rgb", "rgba", "rgb7"):
                px = c9[_blocks(rng, w, h, 9)]
                px[rng.integers(0, h, 12), rng.integers(0, w, 12)] = rng.integers(0, 256, size=(12, 3))  # antialiased edges
                if kind == "rgba":
                    px = np.concatenate([px, rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8)], axis=2)
                data = R.encode(px, 6 if kind == "rgba" else 2, 8, 1 if kind == "rgb7" else 0, filters=ft)
            elif kind == "pal4":
                data = R.encode(_blocks(rng, w, h, 13).astype(np.uint8), 3, 4, palette=pal4, filters=ft)
            elif kind == "pal8":
                data = R.encode(_blocks(rng, w, h, 200).astype(np.uint8), 3, 8, trns=bytes(rng.integers(0, 256, 150, dtype=np.uint8)),
                                palette=pal8, filters=ft)
            else:
                data = R.encode(_blocks(rng, w, h, 4).astype(np.uint8), 0, 2, filters=ft)
            files.append((data, (w, h)))
        _D.update(files=files, pal4=pal4, pal8=pal8)
        # the shared map: about half of every file's colours
        keys = []
        for data, _ in files:
            st, px, _ = CR.rgb(data)
            assert st == 0
            keys += [int(k) for k in np.unique(CR.pack(px))[::2]]
        _D["keys"] = list(dict.fromkeys(keys))
    return _D


@pytest.fixture(scope="module")
def files():
    return _data()["files"]


_REF = {}


def _ref(data):
    if data not in _REF:
        _REF[data] = CR.rgb(data)
    return _REF[data]


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _q(m):
    return WR.quantise((1, 0, 0, 0, 1, 0) if m is None else [v for r in m for v in r])


def _values(keys, dtype, seed=0):
    top = {"uint8": 255, "uint16": 65535}.get(dtype)  # (the top value is kept for `missing`)
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, top, len(keys)) if top else rng.integers(-2 ** 31, 2 ** 31, len(keys))
    return {int(k): int(v) for k, v in zip(keys, vals)}


def _as_colors(m):
    return np.array(list(m.keys()), dtype=np.uint32), np.array(list(m.values()), dtype=np.int64)


def _warps(api, files, size, seed, boxes=None):
    """one matrix per file: the identity (None), a flip with a quarter turn, then random rotations / scales / shears / shifts"""
    rng = np.random.default_rng(seed)
    ws = []
    for k, (_, wh) in enumerate(files):
        if boxes is not None and boxes[k] is not None:
            wh = boxes[k][2:]
        if k == 0:
            ws.append(None)
        elif k == 1:
            ws.append(api.png_warp_matrix(wh, size, hflip=True, angle=90))
        else:
            ws.append(api.png_warp_matrix(wh, size, angle=float(rng.uniform(-180, 180)), scale=float(rng.uniform(0.5, 4.0)),
                                          shear=(float(rng.uniform(-15, 15)), float(rng.uniform(-15, 15))),
                                          translate=(float(rng.uniform(-4, 4)), float(rng.uniform(-4, 4))), vflip=bool(k % 2)))
    return ws


def _check(api, datas, size, dtype, warps, border, border_label, maps=None, missing=-1, boxes=None, fill=None):
    """maps: None (PACK), one dict {key: value}, or a list of one dict per file -> (statuses, unmatched, tensor as numpy)"""
    colors = None if maps is None else [_as_colors(m) for m in maps] if isinstance(maps, list) else _as_colors(maps)
    st, t, infos, um = api.png_decode_batch_color_labels(datas, size, colors, missing, dtype, boxes=boxes, fill=fill, warp=warps,
                                                         border=border, border_label=border_label)
    got = _np(t)
    assert got.shape == (len(datas),) + tuple(size) and got.dtype == CR.DTYPES[dtype]
    for i, data in enumerate(datas):
        rst, px, inf = _ref(data)
        box = boxes[i] if boxes is not None else None
        m = _q(warps[i])
        want = rst
        if inf["width"] and inf["bit_depth"] == 16:
            want = CR.E_LABEL
        elif inf["width"] and CR.LR.box_error(box, inf["width"], inf["height"]):
            want = CR.E_BOX
        elif inf["width"] and m is None:
            want = CW.E_WARP
        assert st[i] == want, (i, inf, st[i], want)
        if st[i] != 0:
            assert um[i] == 0, i
            if fill is not None:
                assert (got[i] == np.array(fill).astype(got.dtype)).all(), (i, "a failed file's slot was written")
            continue
        assert infos[i] == inf, i
        mp = maps[i] if isinstance(maps, list) else maps
        exp, miss = CW.warp_color_labels(px, size, m, BORDERS[border], border_label or 0, box, mp, missing, dtype)
        assert got[i].tobytes() == exp.tobytes(), (i, inf, size, dtype, border, box, np.argwhere(got[i] != exp)[:4])
        assert um[i] == miss, (i, um[i], miss)
    return st, um, got


@pytest.mark.parametrize("border", ["constant", "clamp"])
@pytest.mark.parametrize("size", SIZES)
def test_random_matrices_against_the_restatement(api, files, size, border):
    """PACK into int64 and MAP into every dtype with the shared map; under "constant" border_label == missing for the 8- and
    16-bit dtypes (the border elements are not counted), the ignore index -1 / -100 for the wide ones"""
    datas = [d for d, _ in files]
    ws = _warps(api, files, size, 11 + size[1])
    const = border == "constant"
    _check(api, datas, size, "int64", ws, border, -100 if const else None)
    total = 0
    for dtype, missing, bl in (("uint8", 255, 255), ("uint16", 65535, 65535), ("int32", -1, -1), ("int64", -1, -100)):
        _, um, _ = _check(api, datas, size, dtype, ws, border, bl if const else None, _values(_data()["keys"], dtype), missing)
        total += sum(um)
    assert total > 0


def test_boxes_and_several_tasks_per_image(api, files):
    """per-image crops at non-zero offsets (one of a single pixel) into 64 x 96: two tasks per image"""
    datas = [d for d, _ in files]
    boxes = [(5, 7, 50, 30), None, (32, 16, 1, 1), (1, 2, 40, 27), None, (30, 0, 7, 29)]
    ws = _warps(api, files, (64, 96), 5, boxes)
    for border, bl in (("constant", 7), ("clamp", None)):
        _, um, _ = _check(api, datas, (64, 96), "int32", ws, border, bl, _values(_data()["keys"], "int32"), -1, boxes=boxes)
        assert max(um) > 0
        _check(api, datas, (64, 96), "int32", ws, border, bl, boxes=boxes)


def test_identity_flips_and_quarter_turns_are_numpy(api, files):
    """the matrices the header lists against numpy.flip / numpy.rot90 of the UN-WARPED call's result at the crop's size, and
    the same `unmatched`"""
    mp = _values(_data()["keys"], "int64")
    for (data, (w, h)), box in zip(files[:4], (None, (3, 5, 20, 11), None, (44, 29, 1, 1))):
        cw, chh = (box[2], box[3]) if box else (w, h)
        _, plain, _, um0 = api.png_decode_batch_color_labels([data], (chh, cw), _as_colors(mp), -1, "int64", boxes=[box])
        plain = _np(plain)[0]
        turns = {"identity": (((1, 0, 0), (0, 1, 0)), lambda d: d, (chh, cw)),
                 "hflip": (((-1, 0, cw), (0, 1, 0)), lambda d: np.flip(d, 1), (chh, cw)),
                 "vflip": (((1, 0, 0), (0, -1, chh)), lambda d: np.flip(d, 0), (chh, cw)),
                 "rot90": (((0, -1, cw), (1, 0, 0)), lambda d: np.rot90(d, 1), (cw, chh)),
                 "rot180": (((-1, 0, cw), (0, -1, chh)), lambda d: np.rot90(d, 2), (chh, cw)),
                 "rot270": (((0, 1, 0), (-1, 0, chh)), lambda d: np.rot90(d, 3), (cw, chh))}
        for name, (M, fn, size) in turns.items():
            for border in ("constant", "clamp"):
                st, t, _, um = api.png_decode_batch_color_labels([data], size, _as_colors(mp), -1, "int64", boxes=[box], warp=[M],
                                                                 border=border)
                assert st == [0] and np.array_equal(_np(t)[0], fn(plain)) and um == um0, (name, box, border)


def test_integer_translation_shifts_and_fills_with_border_label(api, files):
    data, (w, h) = files[0]
    _, plain, _, _ = api.png_decode_batch_color_labels([data], (h, w), None, dtype="int32")
    plain = _np(plain)[0]
    st, t, _, um = api.png_decode_batch_color_labels([data], (h, w), None, dtype="int32", warp=[((1, 0, 5), (0, 1, -3))], border_label=-9)
    got = _np(t)[0]
    exp = np.full((h, w), -9, dtype=np.int32)
    exp[3:, :w - 5] = plain[:h - 3, 5:]
    assert st == [0] and um == [0] and np.array_equal(got, exp)


def test_the_grid_is_shared_with_the_raw_label_warp(api, files):
    """a palette file decoded by png_decode_batch_labels(warp=M) equals the same file decoded here with the map colour -> index
    and the same M, element for element, under both borders (the palettes' colours are distinct)"""
    D = _data()
    for k, pal in ((2, D["pal4"]), (3, D["pal8"])):
        assert len(set(pal)) == len(pal)
        data, wh = files[k]
        cmap = {(r, g, b): i for i, (r, g, b) in enumerate(pal)}
        for size in ((33, 65), (64, 96)):
            M = _warps(api, [files[k]] * 3, size, 40 + k)[2]
            for border, bl in (("constant", 255), ("clamp", None)):
                st_l, lab, _ = api.png_decode_batch_labels([data], size, "int32", warp=[M], border=border, border_label=bl)
                st_c, col, _, um = api.png_decode_batch_color_labels([data], size, cmap, -1, "int32", warp=[M], border=border, border_label=bl)
                assert st_l == st_c == [0] and um == [0]
                assert np.array_equal(_np(lab), _np(col)), (k, size, border)


def test_per_image_maps(api, files):
    datas = [d for d, _ in files]
    keys = _data()["keys"]
    maps = [_values(keys[i::3], "int64", i) for i in range(len(datas))]
    maps[1] = {}
    ws = _warps(api, files, (33, 65), 3)
    _, um, _ = _check(api, datas, (33, 65), "int64", ws, "constant", -1, maps, -1)
    assert len(set(um)) > 1
    _check(api, datas, (33, 65), "uint16", ws, "clamp", None, [{k: v & 0xFFFF for k, v in m.items()} for m in maps], 65535)


def test_mixed_batch_keeps_fill_in_the_failed_slots(api, files):
    """a 16-bit file (status 15), a bad matrix (status 16) and a truncated file between good ones: their slots keep `fill`"""
    rng = np.random.default_rng(8)
    rgb16 = R.encode(R.random_image(rng, 9, 7, 2, 16), 2, 16)
    cut = files[0][0][: len(files[0][0]) // 2]
    datas = [files[0][0], rgb16, files[2][0], files[5][0], cut, files[1][0]]
    sub = [files[0], (rgb16, (9, 7)), files[2], files[5], files[0], files[1]]
    ws = _warps(api, sub, (33, 65), 21)
    ws[3] = NAN
    for dtype, fill, mp, missing in (("int64", -12345, None, -1), ("uint8", 0xEE, _values(_data()["keys"], "uint8"), 255)):
        st, um, _ = _check(api, datas, (33, 65), dtype, ws, "constant", 3, mp, missing, fill=fill)
        assert st[1] == CR.E_LABEL == 15 and st[3] == CW.E_WARP == 16 and st[4] not in (0, 15, 16) and st[0] == st[2] == st[5] == 0
