"""The label statistics on the MI355X (include/decode_png.h: debig_png_label_stats; csrc/png_label_stats_kernel.inc):
  * test_battery runs the emulator battery tests/test_emu_png_label_stats.py as it is -- the same run() / check(), shapes, cuts,
    grids and BIT FOR BIT comparisons of the raw records with the numpy restatement tests/png_label_stats_ref.py -- with the launch
    seam tests/stage_launch.py switched to the product library, so the kernel also runs with fewer workgroups than tasks and with
    tables kept and replaced inside one workgroup.  Nothing is compared with the emulator, which is neither built nor loaded.  LEFT
    OUT on purpose: the tasks that break a bound, for the reason tests/test_gpu_png_stage_kernels.py gives (wrong on purpose,
    integer predicates that do not depend on the machine, and a wrong predicate on a shared GPU would be an out-of-range access).
  * the whole calls with stats=: png_decode_batch_labels plain, with a LUT, under warp= with a border label of -1 and under
    elastic=; png_decode_batch_color_labels with a map per image and with packed colours.  The restatement is applied to the
    tensor the call returned; tensor, statuses, infos and `unmatched` are byte-identical to the call without stats=.
  * png_label_stats on tensors made in torch, int16 read as uint16, a status that skips an image, DEBIG_STAGE_GRID."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_stats_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
import test_emu_png_label_stats as E  # noqa: E402  (imports neither build nor load the emulator)

pytestmark = pytest.mark.gpu

KERNEL = "png_label_stats"
EXCLUDED = {"test_tasks_that_break_a_bound_are_skipped": "hands the kernel tasks that break a bound on purpose"}
# the cases of which at least one launch must start fewer workgroups than it has tasks
FEWER = {"test_every_dtype_width_and_height", "test_runs_longer_than_one_round_of_the_lanes", "test_patterns",
         "test_flat_images_large_enough_for_every_wavefront", "test_every_cut_grid_and_order_gives_the_same_records",
         "test_tables_of_different_sizes_alternate_through_one_workgroup", "test_an_image_without_tasks_keeps_zero_records"}


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
    monkeypatch.setitem(SL.KERNELS, KERNEL, (SL.IN, SL.OUT, SL.TASKS))
    monkeypatch.setattr(SL, "backend", "gpu")
    monkeypatch.setattr(SL, "record", [])
    monkeypatch.delenv("DEBIG_STAGE_GRID", raising=False)
    return SL.record


def test_every_battery_case_runs_or_is_excluded():
    tests = _battery_tests()
    ran = {c.values[0] for c in _cases()}
    assert ran | set(EXCLUDED) == set(tests) and not ran & set(EXCLUDED) and all(EXCLUDED.values())
    assert FEWER <= ran and len(ran) >= 9


@pytest.mark.parametrize("name,kw", _cases())
def test_battery(name, kw, on_the_gpu):
    _battery_tests()[name](**kw)
    assert on_the_gpu and {r[0] for r in on_the_gpu} == {KERNEL}, (name, "no launch reached the GPU")
    assert any(n > 0 for _, _, n, _ in on_the_gpu)
    if name in FEWER:
        assert any(0 < g < n for _, _, n, g in on_the_gpu), (name, "no launch with fewer workgroups than tasks")


# ---- the whole calls ---------------------------------------------------------------------------------------------------------------------

from test_gpu_png_color_labels_warp import files as clw_files  # noqa: E402,F401  (the fixtures of the calls' own GPU tests)
from test_gpu_png_labels import datas as label_datas  # noqa: E402,F401


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _bytes(v):
    import torch

    if isinstance(v, torch.Tensor):
        raw = v.contiguous().view(torch.uint8).cpu().numpy() if v.numel() else np.zeros(0, np.uint8)
        return (str(v.dtype), tuple(v.shape), raw.tobytes())
    if isinstance(v, (list, tuple)):
        return [_bytes(e) for e in v]
    if isinstance(v, dict):
        return {k: _bytes(e) for k, e in v.items()}
    return v


def _whole(call, K, n_good, n_bad):
    """call(stats) without and with stats=K: everything but the last element byte-identical, the records those of the restatement
    on the tensor that came back, zero for the failed files -> (statuses, tensor as numpy, records, the rest of the result)"""
    plain = call(None)
    got = call(K)
    assert isinstance(got, tuple) and len(got) == len(plain) + 1 and _bytes(got[:-1]) == _bytes(plain)
    st, rec = got[0], got[-1]
    lab = _np(got[1])
    assert isinstance(rec, np.ndarray) and rec.dtype == np.int64 and rec.shape == (len(st), K + 1, 5)
    assert sum(s == 0 for s in st) >= n_good and sum(s != 0 for s in st) >= n_bad
    want = R.stats(lab, K, st)
    assert np.array_equal(rec, want), np.argwhere(rec != want)[:6]
    for i, s in enumerate(st):
        if s != 0:
            assert not rec[i].any(), (i, "a failed file has records")
        else:
            assert rec[i, :, 0].sum() == lab.shape[1] * lab.shape[2]
    return st, lab, rec, got[2:-1]


@pytest.mark.parametrize("with_lut", [False, True])
@pytest.mark.parametrize("dtype", ["int64", "uint8"])
def test_labels_plain_and_with_a_lut(api, label_datas, dtype, with_lut):
    import test_gpu_png_labels as G

    lut = G.LUT if with_lut else None
    for size in ((75, 50), (32, 24)):
        st, lab, rec, _ = _whole(lambda s: api.png_decode_batch_labels(label_datas, size, dtype=dtype, lut=lut, fill=9, stats=s), 21, 8, 3)
        assert (rec[:, :21, 0].sum(axis=1) > 0).sum() >= 4 and rec[:, 21, 0].sum() > 0  # ids below 21 and "other" both occur


def _fit(api, datas, size, **kw):
    return [api.png_warp_matrix((inf["width"], inf["height"]), size, **kw) for inf in (api.png_info(d)[1] for d in datas)]


def test_labels_under_a_warp_the_border_lands_in_other(api, label_datas):
    size = (40, 56)
    ws = _fit(api, label_datas, size, angle=30.0, scale=0.8, translate=(2.0, -1.5))
    for dtype in ("int64", "int32"):
        st, lab, rec, _ = _whole(lambda s: api.png_decode_batch_labels(label_datas, size, dtype=dtype, fill=9, warp=ws, border="constant",
                                                                       border_label=-1, stats=s), 21, 8, 3)
        good = [i for i, s in enumerate(st) if s == 0]
        border = np.array([(lab[i] == -1).sum() for i in good])
        assert (border > 0).sum() >= 8 and (rec[good, 21, 0] >= border).all()  # (a 1 x 1 file turned by 30 degrees may have none)


def test_labels_under_an_elastic_field(api, label_datas):
    size = (48, 40)
    field = api.png_elastic_field(size, alpha=6.0, sigma=7.0, rng=4)
    _whole(lambda s: api.png_decode_batch_labels(label_datas, size, dtype="uint16", fill=9, elastic=[field] * len(label_datas),
                                                 border="constant", border_label=65535, warp=_fit(api, label_datas, size, scale=0.9), stats=s),
           256, 8, 3)


def _maps_below(K, keys, n):
    rng = np.random.default_rng(K)
    return [{int(k): int(v) for k, v in zip(keys[i::3], rng.integers(0, K, len(keys[i::3])))} for i in range(n)]


@pytest.mark.parametrize("dtype,missing", [("int64", -1), ("uint16", 65535)])
def test_colour_labels_with_a_map_per_image(api, clw_files, dtype, missing):
    import test_gpu_png_color_labels_warp as G

    K = 21
    datas = [d for d, _ in clw_files] + [b"not a png"]
    maps = _maps_below(K, G._data()["keys"], len(datas))
    maps[1] = {}
    colors = [G._as_colors(m) for m in maps]
    st, lab, rec, rest = _whole(lambda s: api.png_decode_batch_color_labels(datas, (33, 65), colors, missing, dtype, fill=5, stats=s), K, 5, 1)
    unmatched = rest[1]
    assert len(set(unmatched)) > 2 and unmatched[1] == 33 * 65
    for i, s in enumerate(st):  # every value of the maps is an id: "other" is exactly what no key matched
        assert rec[i, K, 0] == unmatched[i], i


def test_colour_labels_under_a_warp_and_an_elastic_field(api, clw_files):
    import test_gpu_png_color_labels_warp as G

    K, size = 21, (33, 65)
    datas = [d for d, _ in clw_files]
    colors = [G._as_colors(m) for m in _maps_below(K, G._data()["keys"], len(datas))]
    ws = G._warps(api, clw_files, size, 3)
    ws[2] = G.NAN  # (status 16 in the middle of the batch)
    st, lab, rec, rest = _whole(lambda s: api.png_decode_batch_color_labels(datas, size, colors, -1, "int64", fill=5, warp=ws, border="constant",
                                                                            border_label=-1, stats=s), K, 4, 1)
    assert all(rec[i, K, 0] >= rest[1][i] for i in range(len(datas)))  # the border picks are "other" too, and are not `unmatched`
    field = api.png_elastic_field(size, alpha=4.0, sigma=6.0, rng=2)
    _whole(lambda s: api.png_decode_batch_color_labels(datas, size, colors, -1, "int32", fill=5, warp=ws, elastic=[field] * len(datas),
                                                       border="clamp", stats=s), K, 4, 1)
    _whole(lambda s: api.png_decode_batch_color_labels(datas, size, colors, -1, "int32", fill=5, stats=s,
                                                       perspective=[api.png_perspective_from_warp(w) if w is not None and w is not G.NAN else None
                                                                    for w in ws]), K, 5, 0)


def test_packed_colours_are_nearly_all_other(api, clw_files):
    datas = [d for d, _ in clw_files] + [b""]
    st, lab, rec, _ = _whole(lambda s: api.png_decode_batch_color_labels(datas, (64, 96), None, dtype="int64", fill=5, stats=s), 16, 5, 1)
    good = [i for i, s in enumerate(st) if s == 0]
    assert (rec[good, 16, 0] > 0.5 * 64 * 96).sum() >= 4
    assert (rec[good, 16, 1:] == [0, 0, 96, 64]).all(axis=1).sum() >= 4  # "other" spans the whole image


# ---- png_label_stats on tensors made in torch --------------------------------------------------------------------------------------------

def _torch_dtypes():
    import torch

    return {"uint8": torch.uint8, "uint16": torch.int16, "int32": torch.int32, "int64": torch.int64}


@pytest.mark.parametrize("shape", [(3, 1, 1), (2, 24, 33), (1, 300, 70)])
@pytest.mark.parametrize("name", ["uint8", "uint16", "int32", "int64"])
def test_tensors_made_in_torch(api, gpu_device, name, shape):
    import torch

    rng = np.random.default_rng(shape[2])
    small = rng.integers(0, 30, (shape[0], -(-shape[1] // 4), -(-shape[2] // 6)))
    lab = np.repeat(np.repeat(small, 4, axis=1), 6, axis=2)[:, :shape[1], :shape[2]].astype(E.DTYPES[name][1])
    flat = lab.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = np.iinfo(lab.dtype).max  # stray pixels at the top of the dtype
    if lab.dtype.kind == "i":
        flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = np.iinfo(lab.dtype).min
    if name == "int64":
        flat[rng.integers(0, flat.size, 2)] = 2 ** 32 + 3
    host = lab.view(np.int16) if name == "uint16" else lab  # uint16 as the library hands it out where torch has none
    t = torch.from_numpy(host.copy()).to(gpu_device)
    assert t.dtype == _torch_dtypes()[name]
    for K in (21, 1024):
        got = api.png_label_stats(t, K)
        assert got.dtype == np.int64 and np.array_equal(got, R.stats(lab, K))
    if name == "uint16":
        assert (host < 0).any() and got[:, 1024, 0].sum() >= (host < 0).sum()
    assert t.cpu().numpy().tobytes() == host.tobytes()
    if shape[0] == 3:  # a status that skips the middle image
        got = api.png_label_stats(t, 40, status=[0, 15, 0])
        assert np.array_equal(got, R.stats(lab, 40, [0, 15, 0])) and not got[1].any() and got[0].any() and got[2].any()
        with pytest.raises(ValueError, match="one entry"):
            api.png_label_stats(t, 40, status=[0, 0])
    with pytest.raises(ValueError, match="contiguous"):
        api.png_label_stats(t.transpose(1, 2) if shape[1] > 1 else t.expand(3, 2, 1), 21)
    with pytest.raises(ValueError, match="uint8, uint16"):
        api.png_label_stats(t.to(torch.float32), 21)
    assert api.png_label_stats(t[:0], 21).shape == (0, 22, 5)


def test_the_grid_override_changes_nothing(api, gpu_device, monkeypatch):
    import torch

    rng = np.random.default_rng(6)
    lab = np.repeat(rng.integers(-1, 24, (5, 300, 14)), 5, axis=2).astype(np.int32)  # two tasks per image: ten tasks
    t = torch.from_numpy(lab).to(gpu_device)
    monkeypatch.delenv("DEBIG_STAGE_GRID", raising=False)
    plain = api.png_label_stats(t, 21)
    monkeypatch.setenv("DEBIG_STAGE_GRID", "3")
    three = api.png_label_stats(t, 21)
    monkeypatch.delenv("DEBIG_STAGE_GRID")
    assert plain.tobytes() == three.tobytes() and np.array_equal(plain, R.stats(lab, 21))
