"""debig_png_color_label_kernel (csrc/png_color_label_kernel.inc) on the CPU lock-step emulator, against
tests/png_color_label_ref.py: synthetic RGB8 sources at odd byte offsets into all four dtypes (MAP) and both PACK dtypes, output
widths 1, 7, 9 and 33, several tasks per image, boxes at each corner, a 1-pixel-wide box, enlarging 40 x; maps of 0, 1 and 2048
keys, the keys 0x000000 and 0xFFFFFF, 64 keys that share one slot, per-image maps whose tasks alternate between two tables;
`unmatched` exact; a 4 KiB sentinel kept before and after the tensor; tasks that break a bound are skipped."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_label_ref as CR  # noqa: E402
import png_label_ref as LR  # noqa: E402
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402

FILL = 0xEE
PACK, MAP = 0, 1


class ColorLabelTask(C.Structure):  # include/debig_hip.h: debig_png_color_label_task
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("sx_off", C.c_uint64), ("sy_off", C.c_uint64),
                ("map_off", C.c_uint64), ("src_pitch", C.c_uint32), ("out_w", C.c_uint32), ("out_h", C.c_uint32),
                ("row0", C.c_uint32), ("rows", C.c_uint32), ("map_slots", C.c_uint32), ("missing", C.c_int32),
                ("image", C.c_uint32), ("dtype", C.c_uint8), ("mode", C.c_uint8), ("reserved", C.c_uint16),
                ("reserved2", C.c_uint32)]


assert C.sizeof(ColorLabelTask) == 80
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu(asan=os.environ.get("DEBIG_SPEC_EMU_ASAN") == "1")
        L.emu_png_color_label_batch.restype = C.c_int
        L.emu_png_color_label_batch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def _aligned(nbytes, fill):
    raw = np.full(nbytes + 16, fill, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off: off + nbytes]


def run_gather(srcs, jobs, size, dtype, maps=None, missing=-1, run=None, grid=0):
    """srcs: [(h, w, 3) uint8]; jobs: [(source index, box or None, map index)]; maps: None (PACK) or [{key: value}] ->
    ((len(jobs), H, W) of dtype, unmatched list).  Tables and tasks are made as the host makes them (run: output rows per
    task, default the host's 16384 elements); every source starts at an odd byte of the arena"""
    H, W = size
    es = np.dtype(CR.DTYPES[dtype]).itemsize
    arena, soff = bytearray(16), []
    for s in srcs:
        arena += bytes(-len(arena) % 16 + 1 + 2 * (len(soff) % 3))
        soff.append(len(arena))
        arena += np.ascontiguousarray(s).tobytes()
    tables, axis, moff = bytearray(), {}, []
    for m in maps or []:
        t = CR.table(list(m.keys()), list(m.values()))
        moff.append((len(tables), len(t)))
        tables.extend(t.tobytes())

    def table(cl, L):
        if (cl, L) not in axis:
            axis[(cl, L)] = len(tables)
            t = np.zeros((L + 3) // 4 * 4, dtype=np.uint32)
            t[:L] = LR.index(cl, L)
            tables.extend(t.tobytes())
        return axis[(cl, L)]

    run = run or max(1, 16384 // W)
    tasks = []
    for k, (si, box, mi) in enumerate(jobs):
        h, w = srcs[si].shape[:2]
        x, y, bw, bh = box or (0, 0, w, h)
        for y0 in range(0, H, run):
            t = ColorLabelTask(src_off=soff[si] + (y * w + x) * 3, out_off=k * H * W * es, sx_off=table(bw, W), sy_off=table(bh, H),
                               src_pitch=w, out_w=W, out_h=H, row0=y0, rows=min(run, H - y0), image=k,
                               dtype=list(CR.DTYPES).index(dtype), mode=PACK if maps is None else MAP)
            if maps is not None:
                t.map_off, t.map_slots = moff[mi]
                t.missing = missing
            tasks.append(t)
    n = len(tasks)
    a = np.frombuffer(bytes(arena), dtype=np.uint8).copy()  # (exactly as long as the last source: ASan sees a read past it)
    tb = _aligned(len(tables), 0)
    tb[:] = np.frombuffer(bytes(tables), dtype=np.uint8)
    slot = H * W * es
    out = _aligned(4096 + len(jobs) * slot + 4096, FILL)
    cnt = np.zeros(len(jobs) + 2, dtype=np.uint32)
    cnt[0] = cnt[-1] = 0xDEAD
    assert launch("png_color_label", a, out[4096:], (ColorLabelTask * n)(*tasks), tb, cnt[1:] if maps is not None else None, n, grid,
                  emu=_emu) == 0
    assert (out[:4096] == FILL).all() and (out[4096 + len(jobs) * slot:] == FILL).all(), "the sentinel around the tensor was written"
    assert cnt[0] == 0xDEAD and cnt[-1] == 0xDEAD
    return out[4096: 4096 + len(jobs) * slot].view(CR.DTYPES[dtype]).reshape(len(jobs), H, W), cnt[1:-1].tolist()


def check(srcs, jobs, size, dtype, maps=None, missing=-1, **kw):
    got, um = run_gather(srcs, jobs, size, dtype, maps, missing, **kw)
    for k, (si, box, mi) in enumerate(jobs):
        exp, miss = CR.gather(srcs[si], size, box, None if maps is None else maps[mi], missing, dtype)
        assert got[k].dtype == exp.dtype and got[k].tobytes() == exp.tobytes(), (dtype, size, box, mi, np.argwhere(got[k] != exp)[:4])
        assert um[k] == miss, (dtype, size, box, mi, um[k], miss)
    return got, um


BOXES = [None, (0, 0, 10, 12), (35, 0, 10, 12), (0, 58, 10, 12), (35, 58, 10, 12), (20, 5, 1, 60), (44, 69, 1, 1)]
_SRC = {}


def _colours(rng, n):
    """n distinct packed colours, 0x000000 and 0xFFFFFF among them"""
    ks = {0x000000, 0xFFFFFF}
    while len(ks) < n:
        ks.add(int(rng.integers(0, 1 << 24)))
    return sorted(ks)


def _unpack(keys):
    k = np.asarray(keys, dtype=np.uint32)
    return np.stack([k & 255, (k >> 8) & 255, k >> 16], axis=-1).astype(np.uint8)


def _sources():
    """"blocky": 70 x 45 of 5 x 4 blocks in 7 colours with single stray pixels; "noisy": every pixel one of 2300 colours"""
    if not _SRC:
        rng = np.random.default_rng(2)
        c7 = _colours(rng, 7)
        idx = np.kron(rng.integers(0, 7, size=(14, 12)), np.ones((5, 4), dtype=np.int64))[:70, :45]
        blocky = _unpack(np.array(c7)[idx])
        blocky[rng.integers(0, 70, 40), rng.integers(0, 45, 40)] = rng.integers(0, 256, size=(40, 3))  # antialiased edges
        c2300 = _colours(rng, 2300)
        noisy = _unpack(np.array(c2300)[rng.integers(0, 2300, size=(70, 45))])
        _SRC.update(blocky=blocky, noisy=noisy, c7=c7, c2300=c2300)
    return _SRC


def _values(keys, dtype, seed=0):
    """distinct-ish values in the dtype's range (negative ones for the signed dtypes)"""
    top = {"uint8": 256, "uint16": 65536}.get(dtype)
    rng = np.random.default_rng(seed)
    if top:
        return {k: int(v) for k, v in zip(keys, rng.integers(0, top, len(keys)))}
    return {k: int(v) for k, v in zip(keys, rng.integers(-2 ** 31, 2 ** 31, len(keys)))}


@pytest.mark.parametrize("dtype", list(CR.DTYPES))
@pytest.mark.parametrize("size", [(1, 1), (5, 7), (301, 9), (67, 33)])
def test_every_dtype_size_and_box(dtype, size):
    """MAP with a map that covers 5 of the 7 colours (and none of the stray pixels); PACK for the two dtypes that take it"""
    S = _sources()
    kw = dict(run=None, grid=0) if size[0] < 60 else dict(run=7, grid=5)
    jobs = [(0, b, 0) for b in BOXES]
    missing = 255 if dtype == "uint8" else 65535 if dtype == "uint16" else -1
    check([S["blocky"]], jobs, size, dtype, [_values(S["c7"][:5], dtype)], missing, **kw)
    if dtype in ("int32", "int64"):
        check([S["blocky"]], jobs, size, dtype, None, **kw)
        check([S["noisy"]], jobs[:3], size, dtype, None, **kw)


def test_enlarging_40_times_and_the_identity():
    S = _sources()
    src = S["noisy"]
    m = _values(S["c2300"][::2], "int64")
    for dtype, maps in (("int64", [m]), ("int32", None), ("uint16", [_values(S["c2300"][::2], "uint16")])):
        got, _ = check([src], [(0, (7, 9, 3, 3), 0), (0, (42, 67, 3, 3), 0)], (120, 120), dtype, maps, 7, run=50)
        if maps is None:
            for k, box in enumerate(((7, 9, 3, 3), (42, 67, 3, 3))):
                assert np.array_equal(got[k][::40, ::40], CR.pack(src[box[1]: box[1] + 3, box[0]: box[0] + 3]))
            same, _ = check([src], [(0, None, 0)], (70, 45), dtype, None)
            assert np.array_equal(same[0], CR.pack(src))


def test_maps_of_0_1_and_2048_keys_and_the_extreme_keys():
    S = _sources()
    size = (23, 33)
    # n = 0: every element is `missing`, unmatched is the whole image
    got, um = check([S["blocky"]], [(0, None, 0), (0, BOXES[4], 0)], size, "int64", [{}], -5, run=5)
    assert (got == -5).all() and um == [23 * 33] * 2
    # n = 1, the key 0xFFFFFF; then 0x000000 alone; then both
    for keys in ([0xFFFFFF], [0x000000], [0x000000, 0xFFFFFF]):
        got, um = check([S["blocky"]], [(0, None, 0)], size, "int32", [{k: 1000 + (k & 1) for k in keys}], -1, run=5)
        assert 0 < um[0] < 23 * 33
    assert 0x000000 in S["c7"] and 0xFFFFFF in S["c7"]
    # 2048 keys (4096 slots, the whole 32 KB): 2048 of the 2300 colours of the noisy source
    for dtype in ("uint8", "int64"):
        m = _values(S["c2300"][:2048], dtype, 3)
        assert CR.slots_for(len(m)) == CR.MAX_SLOTS
        _, um = check([S["noisy"]], [(0, None, 0), (0, BOXES[1], 0)], (70, 45), dtype, [m], 0 if dtype == "uint8" else -1, run=30)
        assert 0 < um[0] < 70 * 45


def test_64_keys_in_one_slot():
    """the longest probe chain: 64 keys (128 slots) that the slot function sends to ONE slot, hit from first to last, and
    misses that walk the whole chain"""
    slots = CR.slots_for(64)
    k = np.arange(1 << 24, dtype=np.uint64)
    h = (((k * 0x9E3779B1) & 0xFFFFFFFF) >> 20) & (slots - 1)
    same = [int(v) for v in k[h == 77][:80]]
    assert len(same) == 80 and all(CR.slot(v, slots) == 77 for v in same)
    keys, others = same[:64], same[64:]  # `others` start in the same slot and are not in the map
    t = CR.table(keys, range(64))
    assert [int(v) for v in t[(77 + np.arange(64)) % slots, 0]] == keys
    rng = np.random.default_rng(9)
    src = _unpack(np.array(keys + others)[rng.integers(0, 80, size=(31, 29))])
    for dtype in ("uint16", "int64"):
        _, um = check([src], [(0, None, 0), (0, (3, 4, 20, 9), 0)], (40, 33), dtype, [{kk: 7 * i for i, kk in enumerate(keys)}], 9999, run=6)
        assert um[0] > 0


def test_per_image_maps_alternate_between_two_tables():
    """consecutive tasks of ONE workgroup (grid 1) alternate between two tables of different sizes -- and between two tables of
    the same size: the re-staging path"""
    S = _sources()
    a, b = _values(S["c7"][:3], "int32", 1), _values(S["c7"][2:], "int32", 2)
    big = _values(S["c2300"][:300], "int32", 4)
    jobs = [(0, None, 0), (1, None, 1), (0, BOXES[2], 0), (1, BOXES[3], 2), (0, None, 1), (0, None, 2)]
    for grid in (1, 2, 0):
        check([S["blocky"], S["noisy"]], jobs, (9, 33), "int32", [a, b, big], -7, run=9, grid=grid)  # one task per job
        check([S["blocky"], S["noisy"]], jobs, (9, 33), "int64", [a, b, big], -7, run=4, grid=grid)  # three tasks per job


def test_tasks_that_break_a_bound_are_skipped():
    S = _sources()
    src = S["blocky"]
    H, W = 6, 20
    m = _values(S["c7"], "int64")
    t = CR.table(list(m.keys()), list(m.values()))
    assert len(t) == 16
    tb = _aligned(128 + 96 + 32, 0)
    tb[:128] = np.frombuffer(t.tobytes(), np.uint8)
    tb[128:].view(np.uint32)[:W] = LR.index(45, W)
    tb[128:].view(np.uint32)[24: 24 + H] = LR.index(70, H)
    base = dict(src_off=17, out_off=0, sx_off=128, sy_off=224, map_off=0, src_pitch=45, out_w=W, out_h=H, row0=0, rows=H, map_slots=16,
                missing=-1, image=0, dtype=3, mode=MAP)
    bad = [dict(out_w=0), dict(out_w=16385), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(row0=2, rows=H - 1), dict(dtype=4),
           dict(mode=2), dict(sx_off=136), dict(sy_off=228), dict(map_off=8), dict(map_slots=0), dict(map_slots=1), dict(map_slots=12),
           dict(map_slots=8192), dict(map_slots=1 << 31), dict(mode=PACK, dtype=0), dict(mode=PACK, dtype=1)]
    a = np.zeros(17 + 70 * 45 * 3, dtype=np.uint8)
    a[17:] = src.reshape(-1)
    out = _aligned(4096 + H * W * 8 + 4096, FILL)
    cnt = np.zeros(1, dtype=np.uint32)
    tasks = [ColorLabelTask(**dict(base, **b)) for b in bad]
    n = len(tasks)
    assert _emu().emu_png_color_label_batch(a.ctypes.data, out.ctypes.data + 4096, (ColorLabelTask * n)(*tasks), tb.ctypes.data,
                                            cnt.ctypes.data, n, 0) == 0
    assert (out == FILL).all() and cnt[0] == 0
    # a MAP task without counters is skipped as well
    ok = ColorLabelTask(**base)
    assert _emu().emu_png_color_label_batch(a.ctypes.data, out.ctypes.data + 4096, (ColorLabelTask * 1)(ok), tb.ctypes.data, None, 1, 0) == 0
    assert (out == FILL).all()
    # the same task within its bounds, behind a skipped one
    both = (ColorLabelTask * 2)(tasks[0], ok)
    assert _emu().emu_png_color_label_batch(a.ctypes.data, out.ctypes.data + 4096, both, tb.ctypes.data, cnt.ctypes.data, 2, 1) == 0
    exp, miss = CR.gather(src, (H, W), None, m, -1, "int64")
    assert out[4096: 4096 + H * W * 8].tobytes() == exp.tobytes() and cnt[0] == miss
    assert (out[:4096] == FILL).all() and (out[4096 + H * W * 8:] == FILL).all()


def test_probing_terminates_on_a_table_without_an_empty_slot():
    """a table a device-pointer caller filled to the brim: a key that is not in it is a miss after `slots` probes"""
    src = _unpack(np.array([[1, 2, 3, 99]], dtype=np.uint32))
    full = np.array([[2, 20], [1, 10]], dtype=np.uint32)  # 2 slots, none unused
    tb = _aligned(16 + 16 + 16, 0)
    tb[:16] = np.frombuffer(full.tobytes(), np.uint8)
    tb[16:32].view(np.uint32)[:] = [0, 1, 2, 3]
    a = np.zeros(1 + 12, dtype=np.uint8)
    a[1:] = src.reshape(-1)
    out = _aligned(16, FILL)
    cnt = np.zeros(1, dtype=np.uint32)
    t = ColorLabelTask(src_off=1, out_off=0, sx_off=16, sy_off=32, map_off=0, src_pitch=4, out_w=4, out_h=1, row0=0, rows=1, map_slots=2,
                       missing=-3, image=0, dtype=2, mode=MAP)
    assert launch("png_color_label", a, out, (ColorLabelTask * 1)(t), tb, cnt, 1, 0, emu=_emu) == 0
    assert out.view(np.int32).tolist() == [10, 20, -3, -3] and cnt[0] == 2


def test_kernel_under_address_sanitizer():
    """the same kernel source under ASan + UBSan (tools/simt_emu/libdebig_emu_asan.so), in a child process"""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import test_emu_png_color_labels as E
S = E._sources()
for dtype, size in (("uint8", (5, 33)), ("uint16", (9, 7)), ("int32", (1, 1)), ("int64", (33, 9))):
    jobs = [(0, b, 0) for b in E.BOXES] + [(1, None, 1), (1, E.BOXES[4], 0)]
    maps = [E._values(S["c7"][:5], dtype), E._values(S["c2300"][:2048], dtype, 3)]
    E.check([S["blocky"], S["noisy"]], jobs, size, dtype, maps, 1, run=4, grid=3)
    if dtype in ("int32", "int64"):
        E.check([S["blocky"], S["noisy"]], jobs, size, dtype, None, run=4)
print("asan ok")
""" % {"root": root}
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", DEBIG_SPEC_EMU_ASAN="1")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "asan ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
