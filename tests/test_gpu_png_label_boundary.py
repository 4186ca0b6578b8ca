"""The label boundary on the MI355X (include/decode_png.h: debig_png_label_boundary; csrc/png_label_boundary_kernel.inc):
  * test_battery runs the emulator battery tests/test_emu_png_label_boundary.py as it is -- the same run() / check(), shapes, tile
    cuts, grids and BIT FOR BIT comparisons with the numpy restatement tests/png_label_boundary_ref.py -- with the launch seam
    tests/stage_launch.py switched to the product library, so the kernel also runs with fewer workgroups than tasks.  Nothing is
    compared with the emulator, which is neither built nor loaded.  LEFT OUT on purpose: the tasks that break a bound, for the
    reason tests/test_gpu_png_stage_kernels.py gives (wrong on purpose, integer predicates that do not depend on the machine, and
    a wrong predicate on a shared GPU would be an out-of-range access).  The seam checks that the inputs and the bytes around
    every buffer are unchanged.
  * the whole call api.png_label_boundary against the restatement on the tensors that png_decode_batch_labels returns plain, under
    warp= with a border label of -1 and under elastic=, and that png_decode_batch_color_labels returns with packed colours in
    int64; the ring fed to png_label_stats lands in "other"; tensors made in torch, int16 read as uint16, a status that skips an
    image in both modes, DEBIG_STAGE_GRID."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_boundary_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
import test_emu_png_label_boundary as E  # noqa: E402  (imports neither build nor load the emulator)

pytestmark = pytest.mark.gpu

KERNEL = "png_label_boundary"
EXCLUDED = {"test_tasks_that_break_a_bound_are_skipped": "hands the kernel tasks that break a bound on purpose"}
# the cases of which at least one launch must start fewer workgroups than it has tasks
FEWER = {"test_every_dtype_width_and_height", "test_corners_and_both_sides_of_every_seam", "test_tiles_of_5_by_3_under_radius_16",
         "test_every_cut_grid_and_order_gives_the_same_bytes", "test_the_largest_tiles_of_the_host_cut",
         "test_a_launch_over_half_the_tiles_writes_only_those", "test_images_without_tasks_keep_the_pattern"}
# ... and the one case that launches nothing (it checks the host's tile arithmetic)
NO_LAUNCH = {"test_the_host_cut_fits_and_32_by_32_always_does"}


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
    assert FEWER <= ran and NO_LAUNCH <= ran and len(ran) >= 10


@pytest.mark.parametrize("name,kw", _cases())
def test_battery(name, kw, on_the_gpu):
    _battery_tests()[name](**kw)
    if name in NO_LAUNCH:
        assert not on_the_gpu
        return
    assert on_the_gpu and {r[0] for r in on_the_gpu} == {KERNEL}, (name, "no launch reached the GPU")
    assert any(n > 0 for _, _, n, _ in on_the_gpu)
    if name in FEWER:
        assert any(0 < g < n for _, _, n, g in on_the_gpu), (name, "no launch with fewer workgroups than tasks")


# ---- the whole call ----------------------------------------------------------------------------------------------------------------------

from test_gpu_png_color_labels_warp import files as clw_files  # noqa: E402,F401  (the fixtures of the calls' own GPU tests)
from test_gpu_png_labels import datas as label_datas  # noqa: E402,F401


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _whole(api, t, status, cases):
    """api.png_label_boundary(t, ...) for every (radius, shape, mode, value) against the restatement on the tensor's own bytes;
    the input stays as it was -> the last result as numpy"""
    lab = _np(t)
    before = lab.copy()
    for radius, shape, mode, value in cases:
        got = api.png_label_boundary(t, radius, shape, mode, value, status=status)
        assert got.device == t.device and got.shape == t.shape and got.dtype == (t.dtype if mode == "ring" else __import__("torch").uint8)
        assert got.data_ptr() != t.data_ptr()
        want = R.apply(lab, radius, shape, mode, value, status)
        assert _np(got).tobytes() == want.tobytes(), (radius, shape, mode, np.argwhere(_np(got) != want)[:5])
    assert _np(t).tobytes() == before.tobytes()
    return _np(got), want


CASES = [(1, "square", "ring", 255), (1, "diamond", "edge", 0), (3, "disk", "ring", 255), (16, "square", "edge", 0)]


def _fit(api, datas, size, **kw):
    return [api.png_warp_matrix((inf["width"], inf["height"]), size, **kw) for inf in (api.png_info(d)[1] for d in datas)]


def test_labels_plain_under_a_warp_and_under_an_elastic_field(api, label_datas):
    size = (75, 50)
    st, t, _ = api.png_decode_batch_labels(label_datas, size, dtype="uint8", fill=9)
    assert sum(s == 0 for s in st) >= 8 and sum(s != 0 for s in st) >= 3
    got, _ = _whole(api, t, st, CASES)
    ws = _fit(api, label_datas, (40, 56), angle=30.0, scale=0.8, translate=(2.0, -1.5))
    st, t, _ = api.png_decode_batch_labels(label_datas, (40, 56), dtype="int64", fill=9, warp=ws, border="constant", border_label=-1)
    lab = _np(t)
    good = [i for i, s in enumerate(st) if s == 0]
    assert sum((lab[i] == -1).any() and (lab[i] != -1).any() for i in good) >= 6  # the border label of -1 is an id like any other
    got, want = _whole(api, t, st, [(2, "square", "ring", 255), (1, "diamond", "edge", 0)])
    assert sum(got[i].any() for i in good) >= 6
    field = api.png_elastic_field((48, 40), alpha=6.0, sigma=7.0, rng=4)
    st, t, _ = api.png_decode_batch_labels(label_datas, (48, 40), dtype="uint16", fill=9, elastic=[field] * len(label_datas), border="constant",
                                           border_label=65535, warp=_fit(api, label_datas, (48, 40), scale=0.9))
    _whole(api, t, st, [(2, "disk", "ring", 65535), (5, "diamond", "edge", 0), (1, "square", "ring", 0)])


def test_packed_colours_in_int64_and_the_ring_lands_in_other(api, clw_files):
    datas = [d for d, _ in clw_files] + [b""]
    st, t, _, _ = api.png_decode_batch_color_labels(datas, (64, 96), None, dtype="int64", fill=5)
    assert st[-1] != 0 and sum(s == 0 for s in st) >= 5
    _whole(api, t, st, [(1, "square", "ring", -1), (2, "disk", "ring", 2 ** 40 + 1), (3, "diamond", "edge", 0)])
    # labels -> png_label_boundary -> png_label_stats: a map per image below 21 ids, a ring of 255, which is "other"
    import test_gpu_png_color_labels_warp as G

    K = 21
    rng = np.random.default_rng(K)
    keys = G._data()["keys"]
    colors = [G._as_colors({int(k): int(v) for k, v in zip(keys, rng.integers(0, K, len(keys)))}) for _ in datas]
    st, t, _, unmatched = api.png_decode_batch_color_labels(datas, (33, 65), colors, 0, "int64", fill=5)
    ring = api.png_label_boundary(t, 2, "square", "ring", 255, status=st)
    plain, ringed = api.png_label_stats(t, K, st), api.png_label_stats(ring, K, st)
    want = R.apply(_np(t), 2, "square", "edge", status=st)
    some = 0
    for i, s in enumerate(st):
        if s != 0:
            assert not ringed[i].any()
            continue
        assert plain[i, K, 0] == 0 and ringed[i, K, 0] == want[i].sum() and ringed[i, :, 0].sum() == 33 * 65
        assert (ringed[i, :K, 0] <= plain[i, :K, 0]).all()
        some += want[i].sum() > 0
    assert some >= 4


def _torch_dtypes():
    import torch

    return {"uint8": torch.uint8, "uint16": torch.int16, "int32": torch.int32, "int64": torch.int64}


@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 24, 33), (1, 150, 200)])
@pytest.mark.parametrize("name", ["uint8", "uint16", "int32", "int64"])
def test_tensors_made_in_torch(api, gpu_device, name, shape):
    import torch

    rng = np.random.default_rng(shape[2])
    small = rng.integers(0, 6, (shape[0], -(-shape[1] // 7), -(-shape[2] // 9)))
    lab = np.repeat(np.repeat(small, 7, axis=1), 9, axis=2)[:, :shape[1], :shape[2]].astype(E.DTYPES[name][1])
    flat = lab.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = np.iinfo(lab.dtype).max  # stray pixels at the top of the dtype
    if name == "int64":
        flat[rng.integers(0, flat.size, 2)] = 2 ** 32 + int(flat[0])
    host = lab.view(np.int16) if name == "uint16" else lab  # uint16 as the library hands it out where torch has none
    t = torch.from_numpy(host.copy()).to(gpu_device)
    assert t.dtype == _torch_dtypes()[name]
    top = int(np.iinfo(lab.dtype).max)
    _whole(api, t, None, [(1, "square", "ring", top), (8, "disk", "edge", 0), (16, "diamond", "ring", 0)])
    if name == "uint16":
        assert api.png_label_boundary(t, 1, "square", "ring", 65535).dtype == torch.int16
        with pytest.raises(ValueError, match="value"):
            api.png_label_boundary(t, value=-1)
    if shape[0] == 3:  # a status that skips the middle image, in both modes
        for mode in ("ring", "edge"):
            got = _np(api.png_label_boundary(t, 2, "square", mode, 7, status=[0, 15, 0]))
            assert got.tobytes() == R.apply(lab, 2, "square", mode, 7, [0, 15, 0]).tobytes()
            assert np.array_equal(got[1], lab[1]) if mode == "ring" else not got[1].any()
        with pytest.raises(ValueError, match="one entry"):
            api.png_label_boundary(t, status=[0, 0])
    with pytest.raises(ValueError, match="contiguous"):
        api.png_label_boundary(t.transpose(1, 2) if shape[1] > 1 else t.expand(3, 2, 1))
    with pytest.raises(ValueError, match="uint8, uint16"):
        api.png_label_boundary(t.to(torch.float32))
    assert api.png_label_boundary(t[:0]).shape == (0,) + shape[1:]
    assert api.png_label_boundary(t[:0], mode="edge").dtype == torch.uint8


def test_the_grid_override_changes_nothing(api, gpu_device, monkeypatch):
    import torch

    rng = np.random.default_rng(6)
    lab = np.repeat(rng.integers(-1, 5, (5, 150, 20)), 10, axis=2).astype(np.int32)  # 64 x 64 tiles: 4 x 3 per image, sixty tasks
    t = torch.from_numpy(lab).to(gpu_device)
    monkeypatch.delenv("DEBIG_STAGE_GRID", raising=False)
    plain = api.png_label_boundary(t, 3, "disk", "ring", 255)
    monkeypatch.setenv("DEBIG_STAGE_GRID", "3")
    three = api.png_label_boundary(t, 3, "disk", "ring", 255)
    monkeypatch.delenv("DEBIG_STAGE_GRID")
    assert _np(plain).tobytes() == _np(three).tobytes() == R.apply(lab, 3, "disk", "ring", 255).tobytes()
