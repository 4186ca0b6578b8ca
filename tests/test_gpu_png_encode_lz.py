"""Level 3 of the PNG encode on the MI355X (include/decode_png.h: debig_png_encode_batch_lz; csrc/png_encode_lz_kernel.inc):
  * test_battery runs the emulator battery tests/test_emu_png_encode_lz.py as it is -- the same run_lz() / check_lz(), inputs, cuts and
    grids, check_task() for every task, THE EXACT CHECK of the token rows against the restated rule, the byte for byte comparison
    with the restated dynamic, fixed or stored block, the recorded digests -- with the launch seam tests/stage_launch.py switched to
    the product library.  Nothing is compared with the emulator, which is neither built nor loaded.  LEFT OUT on purpose: the tasks
    that break a bound, for the reason tests/test_gpu_png_stage_kernels.py, tests/test_gpu_png_encode.py and
    tests/test_gpu_png_encode_dyn.py give (wrong on purpose, integer predicates that do not depend on the machine, and a wrong
    predicate on a shared GPU would be an out-of-range access).  The seam checks that the inputs and the bytes around every buffer
    are unchanged.
  * the whole call api.png_encode_batch_lz at level 3 for every colour type x depth x layout under filters none and adaptive: the
    payload inflated by zlib.decompress is the restated filtered stream, the container and every CRC are right, the header is 78 9C,
    the file is within the bound, and the file gives the input bit for bit through api.png_decode_batch(mode="native",
    depth="native");
  * levels 0 .. 2 against png_encode_batch_dyn, 2049 images of 1 x 1 (the round seam), a mixed batch in which every status occurs,
    level 4 refused, DEBIG_STAGE_GRID, the digests of tests/golden/png_encode_lz.json, recorded from the EMULATOR, and the size
    condition: the two label maps of the issue under filter none are strictly smaller than at level 2."""
import ctypes as C
import hashlib
import inspect
import json
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_encode_dyn_ref as D  # noqa: E402
import png_encode_lz_ref as Z  # noqa: E402
import png_encode_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
import test_emu_png_encode as E  # noqa: E402  (imports neither build nor load the emulator)
import test_emu_png_encode_lz as Q  # noqa: E402
from test_gpu_png_encode import _param_sets, _structured, _tensor, parse  # noqa: E402
from test_gpu_png_encode_dyn import _label_map  # noqa: E402

pytestmark = pytest.mark.gpu

EXCLUDED = {"test_tasks_that_break_a_bound_lz": "hands the lz kernel tasks that break a bound on purpose"}
# the cases of which at least one launch must start fewer workgroups than it has tasks
FEWER = {"test_tasks_not_in_the_launch_keep_their_slots_and_rows", "test_every_flag_and_every_branch_of_the_choice", "test_the_window_edge"}
NEW = {Q.LZ}


def _battery_tests():
    return {name: fn for name, fn in vars(Q).items() if name.startswith("test") and inspect.isfunction(fn) and fn.__module__ == Q.__name__}


def _cases():
    out = []
    for name, fn in _battery_tests().items():
        if name in EXCLUDED:
            continue
        for kw in _param_sets(fn):
            assert set(kw) == set(inspect.signature(fn).parameters), (name, "an argument that no parametrize mark gives")
            out.append(pytest.param(name, kw, id=name[5:] + "".join("-" + str(v) for v in kw.values())))
    return out


@pytest.fixture(autouse=True)
def on_the_gpu(gpu_device, monkeypatch):
    """every launch of this module's tests goes to the product library, and is recorded: [(kernel, tasks, n, grid)]"""
    for k, roles in Q.KERNELS.items():
        monkeypatch.setitem(SL.KERNELS, k, roles)
    monkeypatch.setattr(SL, "backend", "gpu")
    monkeypatch.setattr(SL, "record", [])
    monkeypatch.delenv("DEBIG_STAGE_GRID", raising=False)
    return SL.record


def test_every_battery_case_runs_or_is_excluded():
    tests = _battery_tests()
    ran = {c.values[0] for c in _cases()}
    assert ran | set(EXCLUDED) == set(tests) and not ran & set(EXCLUDED) and all(EXCLUDED.values())
    assert all(name.startswith("test_tasks_that_break_a_bound_") for name in EXCLUDED)
    assert FEWER <= ran and len(ran) >= 13


@pytest.mark.parametrize("name,kw", _cases())
def test_battery(name, kw, on_the_gpu):
    _battery_tests()[name](**kw)
    assert on_the_gpu and {r[0] for r in on_the_gpu} <= set(Q.KERNELS), (name, "a kernel whose launch did not reach the GPU")
    assert any(n > 0 and k in NEW for k, _, n, _ in on_the_gpu), name
    if name in FEWER:
        assert any(0 < g < n and k in NEW for k, _, n, g in on_the_gpu), (name, "no launch with fewer workgroups than tasks")


# ---- the whole call ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


def check_file(data, samples, depth, filt, palette=None, trns=None):
    """one level-3 file against the restatement: container, zlib stream, filtered stream, bound -> the IDAT's body"""
    samples = np.asarray(samples)
    H, W, Cn = samples.shape
    ch = parse(data)
    assert ch[b"IHDR"] == struct.pack(">IIBBBBB", W, H, depth, 3 if palette is not None else R.COLOR_TYPE[Cn], 0, 0, 0) and ch[b"IEND"] == b""
    if palette is not None:
        assert ch[b"PLTE"] == np.asarray(palette, np.uint8).tobytes()
    assert ch.get(b"tRNS") == (None if trns is None else bytes(bytearray(trns)))
    z = ch[b"IDAT"]
    stream = R.filtered_stream(samples, depth, filt)
    assert z[:2] == b"\x78\x9c" and zlib.decompress(z) == stream
    assert z[-4:] == struct.pack(">I", zlib.adler32(stream) & 0xFFFFFFFF)
    assert R.container(W, H, Cn, depth, z, palette, trns) == data
    assert len(data) <= R.bound(W, H, Cn, depth, 0 if palette is None else len(palette), 0 if trns is None else len(trns))
    return z


def restated_file(samples, depth, filt, palette=None):
    """the whole level-3 file from the restatement alone"""
    samples = np.asarray(samples)
    H, W, Cn = samples.shape
    stream = R.filtered_stream(samples, depth, filt)
    bpp = Cn * depth // 8
    cuts = R.chunks(len(stream))
    payload = b"".join(Z.task_bytes(stream, off, ln, bpp, Z.host_stride(W, Cn, depth), k == len(cuts) - 1)[0] for k, (off, ln) in enumerate(cuts))
    return R.container(W, H, Cn, depth, b"\x78\x9c" + payload + struct.pack(">I", zlib.adler32(stream) & 0xFFFFFFFF), palette)


@pytest.mark.parametrize("filt", ["none", "adaptive"])
@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_every_colour_type_depth_and_layout_at_level_3(api, gpu_device, layout, filt):
    imgs, metas = [], []
    for Cn in (1, 2, 3, 4):
        for dtype, depth in (("uint8", 8), ("uint16", 16)):
            for s in (E._rand(Cn + depth, 23 + Cn, 37 - Cn, Cn, depth), _structured(Cn, 30, 41 + Cn, Cn, depth)):
                imgs.append(_tensor(gpu_device, s, dtype, layout))
                metas.append((s, depth))
    res = api.png_encode_batch_lz(imgs, layout=layout, filter=filt)
    assert [st for st, _ in res] == [0] * len(imgs)
    row_above = 0
    for (st, data), (s, depth) in zip(res, metas):
        z = check_file(data, s, depth, R.FILTERS[filt])
        assert data == restated_file(s, depth, R.FILTERS[filt])  # the host's row_stride and chunk cut are the restatement's
        S = Z.host_stride(s.shape[1], s.shape[2], depth)
        row_above += any(d == S for b in D.blocks(z[2:-4]) for _, d in b["matches"])
        st2, got, _, _, _ = R.samples_of(data)
        assert st2 == 0 and np.array_equal(got, s)
    assert row_above >= 1 or filt != "none", "level 3 never matched the row above"
    back = api.png_decode_batch([d for _, d in res], mode="native", depth="native")
    for (st, px, inf), (s, depth) in zip(back, metas):
        assert st == 0 and px.dtype == (np.uint16 if depth == 16 else np.uint8) and np.array_equal(px.astype(np.int64), s)


def test_levels_0_to_2_through_the_new_call_are_the_dyn_call_and_the_grid_changes_no_byte(api, gpu_device, monkeypatch):
    imgs = [_tensor(gpu_device, _structured(k, 150, 160, 3, 8)) for k in range(3)] + [_tensor(gpu_device, E._rand(7, 40, 50, 1, 16), "uint16")]
    for level in (0, 1, 2):
        for filt in ("none", "adaptive"):
            assert api.png_encode_batch_lz(imgs, filter=filt, level=level) == api.png_encode_batch_dyn(imgs, filter=filt, level=level)
    plain = api.png_encode_batch_lz(imgs)
    monkeypatch.setenv("DEBIG_STAGE_GRID", "3")
    three = api.png_encode_batch_lz(imgs)
    monkeypatch.delenv("DEBIG_STAGE_GRID")
    assert plain == three and all(s == 0 for s, _ in plain)
    assert plain != api.png_encode_batch_dyn(imgs)


def test_2049_images_of_one_pixel_cross_the_round_seam(api, gpu_device):
    import torch

    assert D.ROUND_TASKS == 2048
    vals = np.arange(2049) % 251
    t = torch.from_numpy(vals.astype(np.uint8).reshape(2049, 1, 1)).to(gpu_device)
    res = api.png_encode_batch_lz(t, filter="none")
    assert len(res) == 2049 and all(st == 0 for st, _ in res)
    want = {int(v): restated_file(np.array([[[v]]]), 8, 0) for v in set(vals.tolist())}
    for k in (0, 1, 2047, 2048):
        check_file(res[k][1], np.array([[[vals[k]]]]), 8, 0)
    assert all(data == want[int(v)] for (_, data), v in zip(res, vals))


def test_a_mixed_batch_in_which_every_status_occurs(api, gpu_device):
    import torch

    good = [_label_map(k, 60 + k, 90, 9) for k in range(3)]
    bad_range = good[1].copy()
    bad_range[7, 9, 0] = 256
    t_good = [_tensor(gpu_device, g, "int32") for g in good]
    t_five = torch.zeros((4, 6, 5), dtype=torch.uint8, device=gpu_device)  # five channels
    alone = api.png_encode_batch_lz(t_good, depth=8)
    mixed = api.png_encode_batch_lz([t_good[0], _tensor(gpu_device, bad_range, "int32"), t_good[1], t_five, t_good[2]], depth=8)
    assert [s for s, _ in mixed] == [0, R.E_RANGE, 0, R.E_ENCODE, 0] and mixed[1][1] is None and mixed[3][1] is None
    assert [mixed[0][1], mixed[2][1], mixed[4][1]] == [d for _, d in alone]
    for (s_, d), g in zip(alone, good):
        assert s_ == 0
        check_file(d, g, 8, 5)
    # E_OUTPUT through the C call: a cap one below the size, beside a file that fits exactly; level 4 is refused
    from debigulator_amd import _native as N

    L = N.lib()
    size = len(alone[0][1])
    descs = (api.PngEncodeDesc * 2)()
    for d in descs:
        d.width, d.height, d.channels, d.dtype, d.depth = 90, 60, 1, 2, 8
    bufs = [np.full(size + 8, 0xAB, np.uint8) for _ in range(2)]
    sizes, status = (C.c_uint64 * 2)(), (C.c_uint32 * 2)()
    torch.cuda.synchronize()
    L.debig_png_encode_batch_lz.restype = C.c_int
    L.debig_png_encode_batch_lz.argtypes = [C.c_void_p] * 7 + [C.c_uint32] * 3
    args = ((C.c_void_p * 2)(t_good[0].data_ptr(), t_good[0].data_ptr()), descs, None, (C.c_void_p * 2)(*[b.ctypes.data for b in bufs]),
            (C.c_uint64 * 2)(size - 1, size), sizes, status, 2, 5)
    assert L.debig_png_encode_batch_lz(*args, 4) == R.BAD_ARG and (bufs[1] == 0xAB).all()
    rc = L.debig_png_encode_batch_lz(*args, 3)
    assert rc == 0 and list(status) == [R.E_OUTPUT, 0] and list(sizes) == [size, size]
    assert (bufs[0] == 0xAB).all() and bufs[1][:size].tobytes() == alone[0][1] and (bufs[1][size:] == 0xAB).all()
    with pytest.raises(ValueError, match="level"):
        api.png_encode_batch_lz(t_good, level=4)


def _filter_name(filt):
    return [k for k, v in R.FILTERS.items() if v == filt][0]


def test_the_digests_recorded_from_the_emulator(api, gpu_device):
    rec = json.load(open(Q.golden_path()))
    cases = Q.golden_inputs()
    assert sorted(rec) == sorted(c[0] for c in cases)
    for name, im, filt, pal, trns in cases:
        t = _tensor(gpu_device, im.s, im.dtype, im.layout)
        (st, data), = api.png_encode_batch_lz([t], layout=im.layout, depth=im.depth, palette=pal, trns=trns, filter=_filter_name(filt))
        assert st == 0 and hashlib.sha256(data).hexdigest() == rec[name], name


def test_the_two_label_maps_are_strictly_smaller_than_at_level_2(api, gpu_device):
    """THE SIZE CONDITION.  The issue's model gave 0.24 (blocky) and 0.53 (curved borders) of level 2's DEFLATE bytes; those are what
    to expect, not a threshold.  The emulator (tests/test_emu_png_encode_lz.py) gave 0.251 and 0.534 of the level-2 FILE."""
    for name, im, filt, pal, trns in Q.golden_inputs()[-2:]:
        t = _tensor(gpu_device, im.s, im.dtype, im.layout)
        (st3, three), = api.png_encode_batch_lz([t], palette=pal, filter="none")
        (st2, two), = api.png_encode_batch_dyn([t], palette=pal, filter="none")
        print(name, "level 3", len(three), "level 2", len(two), "ratio %.3f" % (len(three) / len(two)))
        assert st3 == 0 and st2 == 0 and len(three) < len(two), name
        check_file(three, im.s, 8, 0, palette=pal)
