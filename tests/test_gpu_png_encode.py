"""The PNG encode on the MI355X (include/decode_png.h: debig_png_encode_batch; csrc/png_encode_kernel.inc):
  * test_battery runs the emulator battery tests/test_emu_png_encode.py as it is -- the same run_*() / check_*(), shapes, cuts, grids,
    the byte for byte comparison of the filter output with the numpy restatement, check_task() for every deflate task, the identical
    bytes under grids 0, 1 and 3 and reversed task order, the recorded digests -- with the launch seam tests/stage_launch.py switched
    to the product library.  Nothing is compared with the emulator, which is neither built nor loaded.  LEFT OUT on purpose: the
    tasks that break a bound, for the reason tests/test_gpu_png_stage_kernels.py gives (wrong on purpose, integer predicates that do
    not depend on the machine, and a wrong predicate on a shared GPU would be an out-of-range access).  The seam checks that the
    inputs and the bytes around every buffer are unchanged.
  * the whole call api.png_encode_batch for every colour type x depth x layout x filter mode x level on random and on structured
    images: the payload inflated by zlib.decompress (which checks the zlib header and the Adler-32) is the restated filtered stream,
    every chunk CRC is right, the chunks are the ones the header promises, and the file gives the input bit for bit through
    api.png_decode_batch(mode="native", depth="native") on the GPU and through tests/png_spec_ref.py;
  * round trips with the project's own tensors, a mixed batch in which every status occurs, the ValueErrors, the empty batch,
    DEBIG_STAGE_GRID, and the digests of tests/golden/png_encode.json, recorded from the EMULATOR: the one place where emulator
    bytes and GPU bytes meet."""
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
import png_encode_ref as R  # noqa: E402
import png_spec_ref as S  # noqa: E402
import stage_launch as SL  # noqa: E402
import test_emu_png_encode as E  # noqa: E402  (imports neither build nor load the emulator)

pytestmark = pytest.mark.gpu

EXCLUDED = {"test_tasks_that_break_a_bound_filter": "hands the filter kernel tasks that break a bound on purpose",
            "test_tasks_that_break_a_bound_deflate": "hands the deflate kernel tasks that break a bound on purpose"}
# the cases of which at least one launch must start fewer workgroups than it has tasks
FEWER = {"test_fewer_workgroups_than_tasks_in_both_orders", "test_images_without_tasks_keep_the_pattern", "test_the_stored_fallback_and_the_all_zero_stream",
         "test_tasks_not_in_the_launch_keep_their_slots"}


def _battery_tests():
    return {name: fn for name, fn in vars(E).items() if name.startswith("test") and inspect.isfunction(fn) and fn.__module__ == E.__name__}


def _param_sets(fn):
    """the argument sets of a test function's parametrize marks, as pytest crosses them"""
    sets = [{}]
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [s.strip() for s in mark.args[0].split(",")]
        sets = [dict(s, **dict(zip(names, v if len(names) > 1 else (v,)))) for v in mark.args[1] for s in sets]
    return sets


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
    for k, roles in E.KERNELS.items():
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
    assert FEWER <= ran and len(ran) >= 18


@pytest.mark.parametrize("name,kw", _cases())
def test_battery(name, kw, on_the_gpu):
    _battery_tests()[name](**kw)
    assert on_the_gpu and {r[0] for r in on_the_gpu} <= set(E.KERNELS), (name, "a kernel whose launch did not reach the GPU")
    assert any(n > 0 for _, _, n, _ in on_the_gpu), name
    if name in FEWER:
        assert any(0 < g < n for _, _, n, g in on_the_gpu), (name, "no launch with fewer workgroups than tasks")


# ---- the whole call ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


def _tensor(dev, samples, dtype="uint8", layout="hwc"):
    """(H, W, C) sample values -> the device tensor of that dtype and layout (uint16 as the int16 bits; one channel: (H, W))"""
    import torch

    a = np.asarray(samples).astype(E.DTYPES[dtype][1])
    a = a[:, :, 0] if a.shape[2] == 1 else a.transpose(2, 0, 1) if layout == "chw" else a
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if dtype == "uint16" else a).to(dev)


def parse(data):
    """a file -> {type: body} after checking the signature, the order IHDR [PLTE] [tRNS] IDAT IEND, every length and every CRC"""
    assert data[:8] == S.SIG
    at, chunks = 8, []
    while at < len(data):
        ln, typ = struct.unpack(">I4s", data[at: at + 8])
        body = data[at + 8: at + 8 + ln]
        assert struct.unpack(">I", data[at + 8 + ln: at + 12 + ln])[0] == zlib.crc32(typ + body) & 0xFFFFFFFF, typ
        chunks.append((typ, body))
        at += 12 + ln
    assert at == len(data)
    names = [t for t, _ in chunks]
    assert names in ([b"IHDR", b"IDAT", b"IEND"], [b"IHDR", b"PLTE", b"IDAT", b"IEND"], [b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND"]), names
    return dict(chunks)


def check_file(data, samples, depth, filt, level, palette=None, trns=None):
    """one file of the call against the restatement: container, zlib stream, filtered stream, size"""
    samples = np.asarray(samples)
    H, W, Cn = samples.shape
    ch = parse(data)
    assert ch[b"IHDR"] == struct.pack(">IIBBBBB", W, H, depth, 3 if palette is not None else R.COLOR_TYPE[Cn], 0, 0, 0) and ch[b"IEND"] == b""
    if palette is not None:
        assert ch[b"PLTE"] == np.asarray(palette, np.uint8).tobytes()
    assert ch.get(b"tRNS") == (None if trns is None else bytes(bytearray(trns)))
    z = ch[b"IDAT"]
    stream = R.filtered_stream(samples, depth, filt)
    assert z[:2] == b"\x78\x01" and zlib.decompress(z) == stream
    assert z[-4:] == struct.pack(">I", zlib.adler32(stream) & 0xFFFFFFFF)
    stored = R.stored_payload(len(stream))
    assert len(z) - 6 == stored if level == 0 else len(z) - 6 <= stored
    assert len(data) <= R.bound(W, H, Cn, depth, 0 if palette is None else len(palette), 0 if trns is None else len(trns))
    assert R.container(W, H, Cn, depth, z, palette, trns) == data
    return z


def _structured(seed, H, W, Cn, depth):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    base = ((x * 3 + y * 5) % (1 << depth))[:, :, None] + rng.integers(0, 1 << depth, (1, 1, Cn))
    img = np.where((x // 8 + y // 8)[:, :, None] % 3 == 0, 7, base) % (1 << depth)
    img[H // 2:, :, :] = img[H // 2 - 1: H // 2, :, :]  # rows equal to the one above
    return img


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("filt", sorted(R.FILTERS, key=R.FILTERS.get))
@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_every_colour_type_depth_layout_filter_and_level(api, gpu_device, layout, filt, level):
    imgs, metas = [], []
    for Cn in (1, 2, 3, 4):
        for dtype, depth in (("uint8", 8), ("uint16", 16)):
            for k, s in enumerate((E._rand(Cn + depth, 23 + Cn, 37 - Cn, Cn, depth), _structured(Cn, 30, 41 + Cn, Cn, depth))):
                imgs.append(_tensor(gpu_device, s, dtype, layout))
                metas.append((s, depth))
    res = api.png_encode_batch(imgs, layout=layout, filter=filt, level=level)
    assert [st for st, _ in res] == [0] * len(imgs)
    for (st, data), (s, depth) in zip(res, metas):
        check_file(data, s, depth, R.FILTERS[filt], level)
        st2, got, _, _, _ = R.samples_of(data)
        assert st2 == 0 and np.array_equal(got, s)
    back = api.png_decode_batch([d for _, d in res], mode="native", depth="native")
    for (st, px, inf), (s, depth) in zip(back, metas):
        assert st == 0 and px.dtype == (np.uint16 if depth == 16 else np.uint8) and np.array_equal(px.astype(np.int64), s)
    # one tensor for the batch gives the files of the list
    s = E._rand(5, 19, 21, 3, 8)
    batch = np.stack([s, s[::-1], s[:, ::-1]])
    one = np.ascontiguousarray(batch.transpose(0, 3, 1, 2) if layout == "chw" else batch).astype(np.uint8)
    import torch

    res = api.png_encode_batch(torch.from_numpy(one).to(gpu_device), layout=layout, filter=filt, level=level)
    for (st, data), want in zip(res, batch):
        assert st == 0
        check_file(data, want, 8, R.FILTERS[filt], level)


def test_a_stream_of_several_chunks_and_level_1_against_level_0(api, gpu_device):
    s = _structured(3, 300, 299, 3, 8)  # 269 400 bytes: nine chunks
    noise = np.random.default_rng(1).integers(0, 256, (120, 130, 4))
    for filt in ("adaptive", "none"):
        out = {}
        for level in (0, 1):
            res = api.png_encode_batch([_tensor(gpu_device, s), _tensor(gpu_device, noise)], filter=filt, level=level)
            out[level] = [check_file(d, img, 8, R.FILTERS[filt], level) for (st, d), img in zip(res, (s, noise))]
        assert len(out[1][0]) < len(out[0][0]) // 4 and len(out[1][1]) <= len(out[0][1])
    back = api.png_decode_batch([res[0][1]], mode="native", depth="native")
    assert back[0][0] == 0 and np.array_equal(back[0][1], s)


def test_round_trips_with_the_label_decodes(api, gpu_device):
    rng = np.random.default_rng(11)
    pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(21)]
    blocky = [np.repeat(np.repeat(rng.integers(0, 21, (6, 8)), 5, axis=0), 6, axis=1) for _ in range(3)]
    files = [S.encode(b[:, :, None], 3, 8, palette=pal, filters=lambda p, y: y % 5) for b in blocky]
    st, t, _ = api.png_decode_batch_labels(files, (30, 48), dtype="uint8")
    assert list(st) == [0, 0, 0]
    res = api.png_encode_batch(t, palette=np.array(pal, np.uint8), filter="none")
    assert [s for s, _ in res] == [0, 0, 0]
    for (s_, d), b in zip(res, blocky):
        check_file(d, b[:, :, None], 8, 0, 1, palette=np.array(pal, np.uint8))
    st2, t2, _ = api.png_decode_batch_labels([d for _, d in res], (30, 48), dtype="uint8")
    assert list(st2) == [0, 0, 0] and np.array_equal(t2.cpu().numpy(), t.cpu().numpy())
    # uint16, and int64 at depth 16
    wide = rng.integers(0, 65536, (2, 30, 48))
    files16 = [S.encode(w[:, :, None], 0, 16) for w in wide]
    for dtype in ("uint16", "int64"):
        st, t, _ = api.png_decode_batch_labels(files16, (30, 48), dtype=dtype)
        res = api.png_encode_batch(t, depth=16)
        assert list(st) == [0, 0] and [s for s, _ in res] == [0, 0]
        st2, t2, _ = api.png_decode_batch_labels([d for _, d in res], (30, 48), dtype=dtype)
        assert list(st2) == [0, 0] and np.array_equal(t2.cpu().numpy(), t.cpu().numpy())
        for (_, d), w in zip(res, wide):
            check_file(d, w[:, :, None], 16, 5, 1)
    # instance ids: labels -> png_label_components (int32) -> a 16-bit grey file
    ids, counts = api.png_label_components(t2, 8)
    res = api.png_encode_batch(ids, filter="none")
    for (s_, d), want in zip(res, ids.cpu().numpy()):
        assert s_ == 0
        check_file(d, want[:, :, None], 16, 0, 1)
    st3, t3, _ = api.png_decode_batch_labels([d for _, d in res], (30, 48), dtype="int32")
    assert np.array_equal(t3.cpu().numpy(), ids.cpu().numpy())


def test_round_trip_with_the_tensor_decode_in_chw(api, gpu_device):
    imgs = [E._rand(k, 40, 52, 3, 8) for k in range(3)]
    files = [S.encode(s, 2, 8) for s in imgs]
    st, t, _ = api.png_decode_batch_tensor(files, (40, 52), mode="rgb", depth=8, dtype="uint", layout="chw", filter="nearest")
    assert list(st) == [0, 0, 0] and tuple(t.shape) == (3, 3, 40, 52)
    assert np.array_equal(t.cpu().numpy().transpose(0, 2, 3, 1), np.stack(imgs))
    res = api.png_encode_batch(t, layout="chw")
    back = api.png_decode_batch([d for _, d in res], mode="native", depth="native")
    for (s_, d), (st2, px, _), want in zip(res, back, imgs):
        assert s_ == 0 and st2 == 0 and np.array_equal(px, want)
        check_file(d, want, 8, 5, 1)
    # a view that is not contiguous is made contiguous
    res2 = api.png_encode_batch(t.permute(0, 2, 3, 1), layout="hwc")
    assert [d for _, d in res2] == [d for _, d in res]


def test_a_mixed_batch_in_which_every_status_occurs(api, gpu_device):
    import torch

    good = [E._rand(k, 20 + k, 31, 1, 8) for k in range(3)]
    bad_range = good[1].copy()
    bad_range[7, 9, 0] = 256
    t_good = [_tensor(gpu_device, g, "int32") for g in good]
    t_range = _tensor(gpu_device, bad_range, "int32")
    t_five = torch.zeros((4, 6, 5), dtype=torch.uint8, device=gpu_device)  # five channels
    alone = api.png_encode_batch(t_good, depth=8)
    mixed = api.png_encode_batch([t_good[0], t_range, t_good[1], t_five, t_good[2]], depth=8)
    assert [s for s, _ in mixed] == [0, R.E_RANGE, 0, R.E_ENCODE, 0] and mixed[1][1] is None and mixed[3][1] is None
    assert [mixed[0][1], mixed[2][1], mixed[4][1]] == [d for _, d in alone]
    for (s_, d), g in zip(alone, good):
        assert s_ == 0
        check_file(d, g, 8, 5, 1)
    # a palette: an index equal to the entries; a negative int64; a uint16 tensor at depth 8
    pal = np.zeros((5, 3), np.uint8)
    idx = torch.tensor([[0, 4], [5, 1]], dtype=torch.uint8, device=gpu_device)
    neg = torch.tensor([[0, -1]], dtype=torch.int64, device=gpu_device)
    res = api.png_encode_batch([idx, idx.clamp(max=4), neg], palette=[pal, pal, None])
    assert [s for s, _ in res] == [R.E_RANGE, 0, R.E_RANGE]
    assert [s for s, _ in api.png_encode_batch([torch.zeros((3, 3), dtype=torch.int16, device=gpu_device)], depth=8)] == [R.E_ENCODE]
    # E_OUTPUT through the C call: a cap one below the size, beside a file that fits exactly
    from debigulator_amd import _native as N

    L = N.lib()
    size = len(alone[0][1])
    descs = (api.PngEncodeDesc * 2)()
    for d in descs:
        d.width, d.height, d.channels, d.dtype, d.depth = 31, 20, 1, 2, 8
    bufs = [np.full(size + 8, 0xAB, np.uint8) for _ in range(2)]
    sizes, status = (C.c_uint64 * 2)(), (C.c_uint32 * 2)()
    torch.cuda.synchronize()
    rc = L.debig_png_encode_batch((C.c_void_p * 2)(t_good[0].data_ptr(), t_good[0].data_ptr()), descs, None,
                                  (C.c_void_p * 2)(*[b.ctypes.data for b in bufs]), (C.c_uint64 * 2)(size - 1, size), sizes, status, 2, 5, 1)
    assert rc == 0 and list(status) == [R.E_OUTPUT, 0] and list(sizes) == [size, size]
    assert (bufs[0] == 0xAB).all() and bufs[1][:size].tobytes() == alone[0][1] and (bufs[1][size:] == 0xAB).all()


def test_value_errors_and_the_empty_batch(api, gpu_device):
    import torch

    t = torch.zeros((2, 4, 5), dtype=torch.uint8, device=gpu_device)
    with pytest.raises(ValueError, match="uint8, uint16"):
        api.png_encode_batch(t.to(torch.float32))
    with pytest.raises(ValueError, match="GPU"):
        api.png_encode_batch(t.cpu())
    with pytest.raises(ValueError, match="tensor"):
        api.png_encode_batch(t[0, 0])
    with pytest.raises(ValueError, match="palette must"):
        api.png_encode_batch(t, palette=np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError, match="filter"):
        api.png_encode_batch(t, filter="best")
    with pytest.raises(ValueError, match="level"):
        api.png_encode_batch(t, level=2)
    assert api.png_encode_batch(t[:0]) == [] and api.png_encode_batch([]) == []


def test_the_grid_override_changes_nothing(api, gpu_device, monkeypatch):
    imgs = [_tensor(gpu_device, _structured(k, 150, 160, 3, 8)) for k in range(4)]  # 72 150 bytes each: three chunks, two runs of rows
    monkeypatch.delenv("DEBIG_STAGE_GRID", raising=False)
    plain = api.png_encode_batch(imgs)
    monkeypatch.setenv("DEBIG_STAGE_GRID", "3")
    three = api.png_encode_batch(imgs)
    monkeypatch.setenv("DEBIG_STAGE_GRID", "1")
    one = api.png_encode_batch(imgs)
    monkeypatch.delenv("DEBIG_STAGE_GRID")
    assert plain == three == one and all(s == 0 for s, _ in plain)
    check_file(plain[2][1], _structured(2, 150, 160, 3, 8), 8, 5, 1)


def test_the_digests_recorded_from_the_emulator(api, gpu_device):
    rec = json.load(open(E.golden_path()))
    cases = E.golden_inputs()
    assert sorted(rec) == sorted(c[0] for c in cases)
    for name, im, filt, level, pal, trns in cases:
        t = _tensor(gpu_device, im.s, im.dtype, im.layout)
        (st, data), = api.png_encode_batch([t], layout=im.layout, depth=im.depth, palette=pal, trns=trns,
                                           filter=[k for k, v in R.FILTERS.items() if v == filt][0], level=level)
        assert st == 0 and hashlib.sha256(data).hexdigest() == rec[name], name
