"""debig_png_color_label_warp_kernel (csrc/png_color_label_warp_kernel.inc) on the CPU lock-step emulator, BIT FOR BIT against
tests/png_color_label_warp_ref.py:
  * output widths 1, 255, 256, 257 and 300 (the lane step to the next item is 256, 1, 1, 0, 0 rows) with a few rows; an output
    of 96 x 64 cut into several tasks per image (more than one atomic per counter), also with fewer workgroups than tasks;
  * a crop of 1 x 1 and crops at a non-zero box offset of a 37 x 29 image (pitch != crop_w, an unaligned src_off), the sources
    at odd bytes of an arena that ends with the last pixel;
  * the flip / quarter-turn matrices, shifts, rotations by odd angles, singular and large-translation matrices (every pick is
    border), under both border modes;
  * maps of 1 key (2 slots) and 2048 keys (4096 slots), 64 keys that share one slot, per-image maps whose tasks alternate
    between two tables in ONE workgroup, a table without an unused slot;
  * PACK into int32 / int64, MAP into all four dtypes; border_label == missing: border elements are not counted;
  * `unmatched` exact, a 4 KiB sentinel kept before and after the tensor, tasks that break a bound are skipped."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_label_ref as CR  # noqa: E402
import png_color_label_warp_ref as CW  # noqa: E402
import test_emu_png_warp as EW  # noqa: E402  (the matrices of the label warp's tests)
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from debigulator_amd.api import png_warp_matrix  # noqa: E402

FILL = 0xEE
PACK, MAP = 0, 1
CONSTANT, CLAMP = CW.CONSTANT, CW.CLAMP


class ColorLabelWarpTask(C.Structure):  # include/debig_hip.h: debig_png_color_label_warp_task
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("map_off", C.c_uint64), ("m", C.c_int64 * 6),
                ("src_pitch", C.c_uint32), ("crop_w", C.c_uint32), ("crop_h", C.c_uint32), ("out_w", C.c_uint32),
                ("out_h", C.c_uint32), ("row0", C.c_uint32), ("rows", C.c_uint32), ("border_label", C.c_int32),
                ("map_slots", C.c_uint32), ("missing", C.c_int32), ("image", C.c_uint32), ("dtype", C.c_uint8), ("mode", C.c_uint8),
                ("border_mode", C.c_uint8), ("reserved", C.c_uint8)]


assert C.sizeof(ColorLabelWarpTask) == 120
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        L.emu_png_color_label_warp_batch.restype = C.c_int
        L.emu_png_color_label_warp_batch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def _aligned(nbytes, fill):
    raw = np.full(nbytes + 16, fill, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off: off + nbytes]


def _task(m, **kw):
    t = ColorLabelWarpTask(**kw)
    t.m[:] = [int(v) for v in m]
    return t


def run_warp(srcs, jobs, size, dtype, maps=None, missing=-1, mode=CONSTANT, border_label=0, run=None, grid=0):
    """srcs: [(h, w, 3) uint8]; jobs: [(source index, box or None, map index, m)]; maps: None (PACK) or [{key: value}] ->
    ((len(jobs), H, W) of dtype, unmatched list).  Tables and tasks as the host makes them (run: output rows per task, default
    the host's 4096 elements); every source starts at an odd byte of the arena, which ends with the last source's last pixel"""
    H, W = size
    es = np.dtype(CR.DTYPES[dtype]).itemsize
    arena, soff = bytearray(16), []
    for s in srcs:
        arena += bytes(-len(arena) % 16 + 1 + 2 * (len(soff) % 3))
        soff.append(len(arena))
        arena += np.ascontiguousarray(s).tobytes()
    tables, moff = bytearray(), []
    for mp in maps or []:
        t = CR.table(list(mp.keys()), list(mp.values()))
        moff.append((len(tables), len(t)))
        tables.extend(t.tobytes())
    run = run or max(1, 4096 // W)
    tasks = []
    for k, (si, box, mi, m) in enumerate(jobs):
        h, w = srcs[si].shape[:2]
        x, y, bw, bh = box or (0, 0, w, h)
        for y0 in range(0, H, run):
            t = _task(m, src_off=soff[si] + (y * w + x) * 3, out_off=k * H * W * es, src_pitch=w, crop_w=bw, crop_h=bh, out_w=W, out_h=H,
                      row0=y0, rows=min(run, H - y0), border_label=border_label, image=k, dtype=list(CR.DTYPES).index(dtype),
                      mode=PACK if maps is None else MAP, border_mode=mode)
            if maps is not None:
                t.map_off, t.map_slots = moff[mi]
                t.missing = missing
            tasks.append(t)
    n = len(tasks)
    a = np.frombuffer(bytes(arena), dtype=np.uint8).copy()
    tb = _aligned(max(len(tables), 16), 0)
    tb[:len(tables)] = np.frombuffer(bytes(tables), dtype=np.uint8)
    slot = H * W * es
    out = _aligned(4096 + len(jobs) * slot + 4096, FILL)
    cnt = np.zeros(len(jobs) + 2, dtype=np.uint32)
    cnt[0] = cnt[-1] = 0xDEAD
    assert launch("png_color_label_warp", a, out[4096:], (ColorLabelWarpTask * n)(*tasks), tb, cnt[1:] if maps is not None else None, n, grid,
                  emu=_emu) == 0
    assert (out[:4096] == FILL).all() and (out[4096 + len(jobs) * slot:] == FILL).all(), "the sentinel around the tensor was written"
    assert cnt[0] == 0xDEAD and cnt[-1] == 0xDEAD
    return out[4096: 4096 + len(jobs) * slot].view(CR.DTYPES[dtype]).reshape(len(jobs), H, W), cnt[1:-1].tolist()


def check(srcs, jobs, size, dtype, maps=None, missing=-1, mode=CONSTANT, border_label=0, **kw):
    got, um = run_warp(srcs, jobs, size, dtype, maps, missing, mode, border_label, **kw)
    for k, (si, box, mi, m) in enumerate(jobs):
        exp, miss = CW.warp_color_labels(srcs[si], size, m, mode, border_label, box, None if maps is None else maps[mi], missing, dtype)
        assert got[k].dtype == exp.dtype and got[k].tobytes() == exp.tobytes(), (dtype, size, box, mi, m, np.argwhere(got[k] != exp)[:4])
        assert um[k] == miss, (dtype, size, box, mi, m, um[k], miss)
    return got, um


# ---- sources, maps, matrices ---------------------------------------------------------------------------------------------------

BOXES = [None, (36, 28, 1, 1), (5, 3, 13, 7), (0, 22, 37, 7), (30, 0, 7, 29)]  # (x, y, w, h) inside the 37 x 29 image
_SRC = {}


def _unpack(keys):
    k = np.asarray(keys, dtype=np.uint32)
    return np.stack([k & 255, (k >> 8) & 255, k >> 16], axis=-1).astype(np.uint8)


def _colours(rng, n):
    ks = {0x000000, 0xFFFFFF}
    while len(ks) < n:
        ks.add(int(rng.integers(0, 1 << 24)))
    return sorted(ks)


def _sources():
    """"blocky": 29 rows x 37 columns of 5 x 4 blocks in 7 colours with single stray pixels; "noisy": every pixel one of 2300"""
    if not _SRC:
        rng = np.random.default_rng(5)
        c7 = _colours(rng, 7)
        idx = np.kron(rng.integers(0, 7, size=(6, 10)), np.ones((5, 4), dtype=np.int64))[:29, :37]
        blocky = _unpack(np.array(c7)[idx])
        blocky[rng.integers(0, 29, 30), rng.integers(0, 37, 30)] = rng.integers(0, 256, size=(30, 3))  # antialiased edges
        c2300 = _colours(rng, 2300)
        noisy = _unpack(np.array(c2300)[rng.integers(0, 2300, size=(29, 37))])
        _SRC.update(blocky=blocky, noisy=noisy, c7=c7, c2300=c2300)
    return _SRC


def _values(keys, dtype, seed=0):
    top = {"uint8": 256, "uint16": 65536}.get(dtype)
    rng = np.random.default_rng(seed)
    if top:
        return {k: int(v) for k, v in zip(keys, rng.integers(0, top, len(keys)))}
    return {k: int(v) for k, v in zip(keys, rng.integers(-2 ** 31, 2 ** 31, len(keys)))}


def _flat(M):
    return [v for r in M for v in r]


def _mats(cw, chh, size):
    """rotations by odd angles about the centres, a shear, a shift that leaves the crop in part, the identity"""
    H, W = size
    ms = [(1, 0, 0, 0, 1, 0), (1, 0, 3, 0, 1, -2),
          _flat(png_warp_matrix((cw, chh), (H, W), angle=17, scale=max(W / cw, H / chh) * 0.8)),
          _flat(png_warp_matrix((cw, chh), (H, W), angle=-133, scale=(W / cw, H / chh), shear=(9, -4))),
          _flat(png_warp_matrix((cw, chh), (H, W), angle=71, scale=2.5 * W / cw, hflip=True))]
    return [EW.q(v) for v in ms]


def _box_wh(src, box):
    return (box[2], box[3]) if box else (src.shape[1], src.shape[0])


# ---- the tests -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [CONSTANT, CLAMP])
@pytest.mark.parametrize("size", [(3, 1), (3, 255), (3, 256), (3, 257), (2, 300)])
def test_every_width_on_every_crop(size, mode):
    """the widths at which a lane's step to its next item changes, on the whole image, a 1 x 1 crop and crops at a box offset;
    MAP with 5 of the 7 colours into int32, PACK into int64"""
    S = _sources()
    src = S["blocky"]
    jobs = [(0, b, 0, m) for b in BOXES for m in _mats(*_box_wh(src, b), size)[1:4]]
    check([src], jobs, size, "int32", [_values(S["c7"][:5], "int32")], -1, mode, -100)
    check([src], jobs, size, "int64", None, mode=mode, border_label=-100)


@pytest.mark.parametrize("dtype", list(CR.DTYPES))
def test_every_dtype_in_several_tasks_per_image(dtype):
    """96 x 64 outputs (H = 64 rows of W = 96) cut into runs of 10 rows: 7 tasks and up to 28 atomics per counter, on as many
    workgroups as tasks and on 3; both border modes; border_label == missing where the dtype has no spare value"""
    S = _sources()
    size = (64, 96)
    missing = 255 if dtype == "uint8" else 65535 if dtype == "uint16" else -1
    jobs = [(si, b, 0, m) for si, b in ((0, None), (0, BOXES[2]), (1, BOXES[3])) for m in _mats(*_box_wh(S["blocky"], b), size)[2:]]
    maps = [_values(S["c7"][:5] + S["c2300"][:40], dtype)]
    for mode, grid in ((CONSTANT, 0), (CLAMP, 3)):
        _, um = check([S["blocky"], S["noisy"]], jobs, size, dtype, maps, missing, mode, missing, run=10, grid=grid)
        assert any(u > 256 for u in um)
    if dtype in ("int32", "int64"):
        check([S["blocky"], S["noisy"]], jobs, size, dtype, None, mode=CONSTANT, border_label=-5, run=10, grid=2)
        check([S["blocky"], S["noisy"]], jobs[:3], size, dtype, None, mode=CLAMP)  # the host's runs: 42 rows


def test_identity_flips_and_quarter_turns_are_numpy():
    """the matrices the header lists reproduce numpy.flip / numpy.rot90 of the un-warped result (the gather restatement at the
    crop's size), unmatched included, under both border modes: no pick leaves the crop"""
    S = _sources()
    src = S["blocky"]
    mp = _values(S["c7"][:4], "int64")
    for box in (None, BOXES[2], BOXES[1]):
        cw, chh = _box_wh(src, box)
        plain, miss = CR.gather(src, (chh, cw), box, mp, -1, "int64")
        for name, (M, fn, size) in EW.flips_and_turns(cw, chh).items():
            for mode in (CONSTANT, CLAMP):
                got, um = check([src], [(0, box, 0, EW.q(M))], size, "int64", [mp], -1, mode, 12345)
                assert np.array_equal(got[0], fn(plain)) and um == [miss], (name, box, mode)
                got, _ = check([src], [(0, box, 0, EW.q(M))], size, "int32", None, mode=mode, border_label=12345)
                assert np.array_equal(got[0], fn(CR.gather(src, (chh, cw), box, None, dtype="int32")[0])), (name, box, mode)


def test_integer_translations_shift_and_fill_with_border():
    S = _sources()
    src, box = S["blocky"], BOXES[2]
    cw, chh = 13, 7
    mp = _values(S["c7"], "int64")
    plain, _ = CR.gather(src, (chh, cw), box, mp, -1, "int64")
    for dx, dy in ((3, -2), (-4, 1), (0, 6), (13, 0), (-20, -20)):
        got, um = check([src], [(0, box, 0, EW.q((1, 0, dx, 0, 1, dy)))], (chh, cw), "int64", [mp], -1, CONSTANT, -7)
        exp = np.full((chh, cw), -7, dtype=np.int64)
        ys, xs = np.arange(chh) + dy, np.arange(cw) + dx
        oky, okx = (ys >= 0) & (ys < chh), (xs >= 0) & (xs < cw)
        exp[np.ix_(oky, okx)] = plain[np.ix_(ys[oky], xs[okx])]
        assert np.array_equal(got[0], exp), (dx, dy)
        assert um == [int((exp == -1).sum())]


@pytest.mark.parametrize("mode", [CONSTANT, CLAMP])
def test_matrices_whose_every_pick_is_border(mode):
    """singular matrices that point outside, translations of +-2^24 and linear entries of +-32768: under CONSTANT the tensor is
    border_label and nothing is counted although border_label == missing; under CLAMP every element is an edge pixel and goes
    through the map"""
    S = _sources()
    src = S["noisy"]
    size = (5, 257)
    ms = [EW.q(v) for v in ((0, 0, -0.5, 0, 0, 3), (0, 0, 5, 0, 0, 29.0), (1, 0, 2.0 ** 24, 0, 1, 2.0 ** 24), (1, 0, -2.0 ** 24, 0, 1, -2.0 ** 24),
                            (32768, 32768, 40, 32768, 32768, 0), (-32768, -32768, -0.25, 32768, -32768, -0.75))]
    jobs = [(0, b, 0, m) for b in (None, BOXES[2]) for m in ms]
    got, um = check([src], jobs, size, "int64", [_values(S["c2300"][::3], "int64")], -1, mode, -1, run=2)
    if mode == CONSTANT:
        assert (got == -1).all() and um == [0] * len(jobs)
    else:
        assert any(u == 5 * 257 for u in um) and any(u == 0 for u in um)  # one edge pixel each: in the map or not
    got, _ = check([src], jobs, size, "int32", None, mode=mode, border_label=-9)
    assert (got == -9).all() == (mode == CONSTANT)
    # the singular matrix that points INTO the crop: one pixel everywhere, no border at all
    inside = EW.q((0, 0, 4.5, 0, 0, 2.5))
    got, um = check([src], [(0, None, 0, inside)], size, "int32", None, mode=mode, border_label=-9)
    assert (got == int(CR.pack(src[2, 4]))).all()


def test_maps_of_1_and_2048_keys():
    S = _sources()
    size = (9, 65)
    for box in (None, BOXES[4]):
        ms = _mats(*_box_wh(S["blocky"], box), size)
        for key in (0x000000, 0xFFFFFF):
            assert CR.slots_for(1) == 2
            _, um = check([S["blocky"]], [(0, box, 0, m) for m in ms], size, "int32", [{key: 1000}], -1, CONSTANT, -1, run=4)
            assert all(0 < u < 9 * 65 for u in um[:2])
        for dtype in ("uint8", "int64"):
            mp = _values(S["c2300"][:2048], dtype, 3)
            assert CR.slots_for(len(mp)) == CR.MAX_SLOTS
            _, um = check([S["noisy"]], [(0, box, 0, m) for m in ms], size, dtype, [mp], 0 if dtype == "uint8" else -1, CLAMP, 0, run=4)
            assert 0 < um[0] < 9 * 65


def test_64_keys_in_one_slot():
    """the longest probe chain: 64 keys (128 slots) that the slot function sends to ONE slot, and misses that walk all of it"""
    slots = CR.slots_for(64)
    k = np.arange(1 << 24, dtype=np.uint64)
    same = [int(v) for v in k[((((k * 0x9E3779B1) & 0xFFFFFFFF) >> 20) & (slots - 1)) == 77][:80]]
    assert len(same) == 80 and all(CR.slot(v, slots) == 77 for v in same)
    keys, others = same[:64], same[64:]
    src = _unpack(np.array(keys + others)[np.random.default_rng(9).integers(0, 80, size=(29, 37))])
    for dtype, mode in (("uint16", CONSTANT), ("int64", CLAMP)):
        jobs = [(0, b, 0, m) for b in (None, BOXES[2]) for m in _mats(*_box_wh(src, b), (11, 70))[1:4]]
        _, um = check([src], jobs, (11, 70), dtype, [{kk: 7 * i for i, kk in enumerate(keys)}], 9999, mode, 9999, run=3)
        assert um[0] > 0


def test_per_image_maps_alternate_between_two_tables_in_one_workgroup():
    """consecutive tasks of ONE workgroup (grid 1) alternate between two tables of different sizes, and between two tables of
    the same size: the re-staging path between its two barriers"""
    S = _sources()
    a, b = _values(S["c7"][:3], "int32", 1), _values(S["c7"][2:5], "int32", 2)
    big = _values(S["c2300"][:300], "int32", 4)
    assert len(CR.table(list(a), list(a.values()))) == len(CR.table(list(b), list(b.values()))) != len(CR.table(list(big), list(big.values())))
    size = (9, 33)
    mw, mb = _mats(37, 29, size), _mats(13, 7, size)
    jobs = [(0, None, 0, mw[2]), (1, None, 1, mw[3]), (0, BOXES[2], 0, mb[2]), (1, BOXES[2], 2, mb[1]), (0, None, 1, mw[4]), (0, None, 2, mw[0])]
    for grid in (1, 2, 0):
        check([S["blocky"], S["noisy"]], jobs, size, "int32", [a, b, big], -7, CONSTANT, -7, run=9, grid=grid)  # one task per job
        check([S["blocky"], S["noisy"]], jobs, size, "int64", [a, b, big], -7, CLAMP, 0, run=4, grid=grid)      # three tasks per job


def test_probing_terminates_on_a_table_without_an_empty_slot():
    """a table a device-pointer caller filled to the brim: a key that is not in it is a miss after `slots` probes"""
    src = _unpack(np.array([[1, 2, 3, 99]], dtype=np.uint32))
    full = np.array([[2, 20], [1, 10]], dtype=np.uint32)  # 2 slots, none unused
    tb = _aligned(16, 0)
    tb[:16] = np.frombuffer(full.tobytes(), np.uint8)
    a = np.zeros(1 + 12, dtype=np.uint8)
    a[1:] = src.reshape(-1)
    out = _aligned(24, FILL)
    cnt = np.zeros(1, dtype=np.uint32)
    t = _task(EW.q((1, 0, 0, 0, 1, 0)), src_off=1, out_off=0, map_off=0, src_pitch=4, crop_w=4, crop_h=1, out_w=6, out_h=1, row0=0,
              rows=1, border_label=-3, map_slots=2, missing=-3, image=0, dtype=2, mode=MAP, border_mode=CONSTANT)
    assert launch("png_color_label_warp", a, out, (ColorLabelWarpTask * 1)(t), tb, cnt, 1, 0, emu=_emu) == 0
    assert out.view(np.int32).tolist() == [10, 20, -3, -3, -3, -3] and cnt[0] == 2  # two misses, two border elements


def test_tasks_that_break_a_bound_are_skipped():
    S = _sources()
    src = S["blocky"]
    H, W = 6, 20
    mp = _values(S["c7"], "int64")
    t = CR.table(list(mp.keys()), list(mp.values()))
    assert len(t) == 16
    tb = _aligned(128, 0)
    tb[:] = np.frombuffer(t.tobytes(), np.uint8)
    ident = EW.q((1, 0, 0, 0, 1, 0))
    base = dict(src_off=17, out_off=0, map_off=0, src_pitch=37, crop_w=37, crop_h=29, out_w=W, out_h=H, row0=0, rows=H, border_label=-2,
                map_slots=16, missing=-1, image=0, dtype=3, mode=MAP, border_mode=CONSTANT)
    bad = [dict(out_w=0), dict(out_w=16385), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(row0=2, rows=H - 1),
           dict(crop_w=0), dict(crop_h=0), dict(crop_w=1 << 31), dict(crop_h=1 << 31), dict(dtype=4), dict(mode=2), dict(border_mode=2),
           dict(map_off=8), dict(map_slots=0), dict(map_slots=1), dict(map_slots=12), dict(map_slots=8192), dict(map_slots=1 << 31),
           dict(mode=PACK, dtype=0), dict(mode=PACK, dtype=1)]
    tasks = [_task(ident, **dict(base, **b)) for b in bad]
    lin, tr = 1 << 31, 1 << 40
    for k in range(6):  # every matrix entry one beyond its limit, both signs
        for sign in (1, -1):
            m = list(ident)
            m[k] = sign * ((tr if k in (2, 5) else lin) + 1)
            tasks.append(_task(m, **base))
    a = np.zeros(17 + 29 * 37 * 3, dtype=np.uint8)
    a[17:] = src.reshape(-1)
    out = _aligned(4096 + H * W * 8 + 4096, FILL)
    cnt = np.zeros(1, dtype=np.uint32)
    n = len(tasks)
    call = _emu().emu_png_color_label_warp_batch
    assert call(a.ctypes.data, out.ctypes.data + 4096, (ColorLabelWarpTask * n)(*tasks), tb.ctypes.data, cnt.ctypes.data, n, 0) == 0
    assert (out == FILL).all() and cnt[0] == 0
    assert call(a.ctypes.data, out.ctypes.data + 4096, (ColorLabelWarpTask * n)(*tasks), tb.ctypes.data, cnt.ctypes.data, n, 2) == 0
    assert (out == FILL).all() and cnt[0] == 0
    # a MAP task without counters is skipped as well
    ok = _task(ident, **base)
    assert call(a.ctypes.data, out.ctypes.data + 4096, (ColorLabelWarpTask * 1)(ok), tb.ctypes.data, None, 1, 0) == 0
    assert (out == FILL).all()
    # the same task within its bounds, behind a skipped one; the matrix entries AT their limits are taken
    both = (ColorLabelWarpTask * 2)(tasks[0], ok)
    assert call(a.ctypes.data, out.ctypes.data + 4096, both, tb.ctypes.data, cnt.ctypes.data, 2, 1) == 0
    exp, miss = CW.warp_color_labels(src, (H, W), ident, CONSTANT, -2, None, mp, -1, "int64")
    assert out[4096: 4096 + H * W * 8].tobytes() == exp.tobytes() and cnt[0] == miss
    assert (out[:4096] == FILL).all() and (out[4096 + H * W * 8:] == FILL).all()
    edge = _task([lin, -lin, tr, -lin, lin, -tr], **base)
    cnt[0] = 0
    assert call(a.ctypes.data, out.ctypes.data + 4096, (ColorLabelWarpTask * 1)(edge), tb.ctypes.data, cnt.ctypes.data, 1, 0) == 0
    exp, miss = CW.warp_color_labels(src, (H, W), [lin, -lin, tr, -lin, lin, -tr], CONSTANT, -2, None, mp, -1, "int64")
    assert out[4096: 4096 + H * W * 8].tobytes() == exp.tobytes() and cnt[0] == miss
