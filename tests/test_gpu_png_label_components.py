"""The label components on the MI355X (include/decode_png.h: debig_png_label_components; csrc/png_label_components_kernel.inc):
  * test_battery runs the emulator battery tests/test_emu_png_label_components.py as it is -- the same run() / check(), shapes, cuts,
    grids, the invariants of the parent plane after the merge launch, every task's count and the BYTE FOR BYTE comparison of both id
    modes with the numpy restatement tests/png_label_components_ref.py -- with the launch seam tests/stage_launch.py switched to the
    product library.  Here the workgroups of the merge launch run side by side, on different XCDs, and update one plane with atomics:
    THIS is what exercises the races, which the emulator (workgroups one after the other) cannot.  Nothing is compared with the
    emulator, which is neither built nor loaded.  LEFT OUT on purpose: the tasks that break a bound and the corrupted parent plane,
    for the reason tests/test_gpu_png_stage_kernels.py gives (wrong on purpose, integer predicates that do not depend on the machine,
    and a wrong predicate on a shared GPU would be an out-of-range access).  The seam checks that the inputs and the bytes around
    every buffer are unchanged.
  * the whole call api.png_label_components against the restatement on the tensors that png_decode_batch_labels returns plain and
    under warp= with a border label of -1, and that png_decode_batch_color_labels returns with packed colours in int64; tensors made
    in torch, int16 read as uint16, a status that skips an image, the ValueErrors, the empty batch, DEBIG_STAGE_GRID;
  * the composition with png_label_stats, and identities on the device: K fixed points under ids="first", the 8-partition coarsens
    the 4-partition, flipping the input flips the partition."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_components_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
import test_emu_png_label_components as E  # noqa: E402  (imports neither build nor load the emulator)

pytestmark = pytest.mark.gpu

EXCLUDED = {"test_tasks_that_break_a_bound_are_skipped": "hands the kernels tasks that break a bound on purpose",
            "test_a_corrupted_parent_plane_ends_cleanly": "hands the kernels a parent plane that is wrong on purpose"}
# the cases of which at least one launch of every kernel must start fewer workgroups than it has tasks
FEWER = {"test_every_dtype_width_height_and_background", "test_row_runs_cut_at_every_seam", "test_fewer_workgroups_than_tasks_in_both_orders",
         "test_a_finish_launch_over_half_the_tasks_writes_only_those", "test_images_without_tasks_keep_the_pattern"}
FIRST_ONLY = {"test_a_finish_launch_over_half_the_tasks_writes_only_those"}  # (ids="first" has no number launch)


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
    assert FEWER <= ran and len(ran) >= 12


@pytest.mark.parametrize("name,kw", _cases())
def test_battery(name, kw, on_the_gpu):
    _battery_tests()[name](**kw)
    kernels = set(E.KERNELS) - ({E.NUMBER} if name in FIRST_ONLY else set())
    assert on_the_gpu and {r[0] for r in on_the_gpu} == kernels, (name, "a kernel whose launch did not reach the GPU")
    for k in kernels:
        assert any(n > 0 for kk, _, n, _ in on_the_gpu if kk == k), (name, k)
        if name in FEWER:
            assert any(0 < g < n for kk, _, n, g in on_the_gpu if kk == k), (name, k, "no launch with fewer workgroups than tasks")


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
    """api.png_label_components(t, ...) for every (connectivity, background, ids) against the restatement on the tensor's own bytes;
    the input stays as it was -> the last result and counts as numpy"""
    import torch

    lab = _np(t)
    before = lab.copy()
    for connectivity, background, ids in cases:
        got, counts = api.png_label_components(t, connectivity, background, ids, status=status)
        assert got.device == t.device and got.shape == t.shape and got.dtype == torch.int32 and got.data_ptr() != t.data_ptr()
        assert isinstance(counts, np.ndarray) and counts.dtype == np.int64 and counts.shape == (lab.shape[0],)
        want, wcounts = R.apply(lab, connectivity, background, ids, status)
        assert _np(got).tobytes() == want.tobytes(), (connectivity, background, ids, np.argwhere(_np(got) != want)[:5])
        assert np.array_equal(counts, wcounts), (connectivity, background, ids, counts, wcounts)
    assert _np(t).tobytes() == before.tobytes()
    return _np(got), counts


def _fit(api, datas, size, **kw):
    return [api.png_warp_matrix((inf["width"], inf["height"]), size, **kw) for inf in (api.png_info(d)[1] for d in datas)]


def test_labels_plain_and_under_a_warp(api, label_datas):
    st, t, _ = api.png_decode_batch_labels(label_datas, (75, 50), dtype="uint8", fill=9)
    assert sum(s == 0 for s in st) >= 8 and sum(s != 0 for s in st) >= 3
    lab = _np(t)
    common = int(np.bincount(lab[[i for i, s in enumerate(st) if s == 0]].ravel()).argmax())
    got, counts = _whole(api, t, st, [(4, None, "consecutive"), (8, common, "first"), (8, None, "first"), (4, common, "consecutive")])
    assert all(not got[i].any() and counts[i] == 0 for i, s in enumerate(st) if s != 0)
    ws = _fit(api, label_datas, (40, 56), angle=30.0, scale=0.8, translate=(2.0, -1.5))
    st, t, _ = api.png_decode_batch_labels(label_datas, (40, 56), dtype="int64", fill=9, warp=ws, border="constant", border_label=-1)
    lab = _np(t)
    good = [i for i, s in enumerate(st) if s == 0]
    assert sum((lab[i] == -1).any() and (lab[i] != -1).any() for i in good) >= 6  # the border label of -1 is an id like any other
    got, counts = _whole(api, t, st, [(4, None, "consecutive"), (8, -1, "first"), (4, -1, "consecutive")])
    assert sum(counts[i] >= 1 for i in good) >= 6 and sum((got[i] == 0).any() for i in good) >= 6


def test_packed_colours_in_int64(api, clw_files):
    datas = [d for d, _ in clw_files] + [b""]
    st, t, _, _ = api.png_decode_batch_color_labels(datas, (64, 96), None, dtype="int64", fill=5)
    assert st[-1] != 0 and sum(s == 0 for s in st) >= 5
    lab = _np(t)
    colour = int(lab[0, 0, 0])
    assert colour > 255 or (lab > 255).any()
    _whole(api, t, st, [(4, None, "consecutive"), (8, colour, "first"), (8, None, "consecutive")])


def _torch_dtypes():
    import torch

    return {"uint8": torch.uint8, "uint16": torch.int16, "int32": torch.int32, "int64": torch.int64}


def _made(name, shape):
    rng = np.random.default_rng(shape[2])
    small = rng.integers(0, 4, (shape[0], -(-shape[1] // 7), -(-shape[2] // 9)))
    lab = np.repeat(np.repeat(small, 7, axis=1), 9, axis=2)[:, :shape[1], :shape[2]].astype(E.DTYPES[name][1])
    flat = lab.reshape(-1)
    top = int(np.iinfo(lab.dtype).max)
    flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = top  # stray pixels at the top of the dtype
    if name == "int64":
        flat[rng.integers(0, flat.size, 4)] = 2 ** 32 + 3  # ... and ids that share their low word with 3
    return lab, top


@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 24, 33), (1, 70, 130)])
@pytest.mark.parametrize("name", ["uint8", "uint16", "int32", "int64"])
def test_tensors_made_in_torch(api, gpu_device, name, shape):
    import torch

    lab, top = _made(name, shape)
    host = lab.view(np.int16) if name == "uint16" else lab  # uint16 as the library hands it out where torch has none
    t = torch.from_numpy(host.copy()).to(gpu_device)
    assert t.dtype == _torch_dtypes()[name]
    _whole(api, t, None, [(4, None, "consecutive"), (8, top, "first"), (8, None, "consecutive"), (4, 0, "first"), (4, 2 ** 40, "consecutive")])
    if shape[0] == 3:  # a status that skips the middle image: zeros and a count of 0, and only there
        got, counts = api.png_label_components(t, 8, 0, "first", status=[0, 15, 0])
        want, wcounts = R.apply(lab, 8, 0, "first", [0, 15, 0])
        assert _np(got).tobytes() == want.tobytes() and not _np(got)[1].any() and counts.tolist() == wcounts.tolist() and counts[1] == 0
        assert counts[0] > 0 and counts[2] > 0
        with pytest.raises(ValueError, match="one entry"):
            api.png_label_components(t, status=[0, 0])
    with pytest.raises(ValueError, match="contiguous"):
        api.png_label_components(t.transpose(1, 2) if shape[1] > 1 else t.expand(3, 2, 1))
    with pytest.raises(ValueError, match="uint8, uint16"):
        api.png_label_components(t.to(torch.float32))
    with pytest.raises(ValueError, match="connectivity"):
        api.png_label_components(t, 6)
    with pytest.raises(ValueError, match="ids"):
        api.png_label_components(t, ids="raster")
    empty, none = api.png_label_components(t[:0])
    assert empty.shape == (0,) + shape[1:] and empty.dtype == torch.int32 and none.shape == (0,) and none.dtype == np.int64


def test_the_grid_override_changes_nothing(api, gpu_device, monkeypatch):
    import torch

    rng = np.random.default_rng(6)
    lab = np.repeat(rng.integers(-1, 3, (6, 90, 20)), 10, axis=2).astype(np.int32)  # two runs of rows per image: 12 tasks
    t = torch.from_numpy(lab).to(gpu_device)
    want, wcounts = R.apply(lab, 8)
    monkeypatch.delenv("DEBIG_STAGE_GRID", raising=False)
    plain, pc = api.png_label_components(t, 8)
    monkeypatch.setenv("DEBIG_STAGE_GRID", "3")
    three, tc = api.png_label_components(t, 8)
    monkeypatch.delenv("DEBIG_STAGE_GRID")
    assert _np(plain).tobytes() == _np(three).tobytes() == want.tobytes() and pc.tolist() == tc.tolist() == wcounts.tolist()


def test_the_composition_with_the_stats_call(api, gpu_device):
    """labels -> png_label_components -> png_label_stats(ids, K + 1): record k has the count and the tight box of ref == k for every
    k in 1 .. K, record 0 the background, and nothing lands in "other" """
    import torch

    lab, _ = _made("int32", (3, 70, 130))
    t = torch.from_numpy(lab).to(gpu_device)
    for connectivity, background in ((4, 0), (8, None)):
        ids, counts = api.png_label_components(t, connectivity, background)
        want, wcounts = R.apply(lab, connectivity, background)
        assert counts.tolist() == wcounts.tolist()
        K = int(counts.max())
        stats = api.png_label_stats(ids, K + 1)
        assert stats.shape == (3, K + 2, 5)
        for i in range(3):
            assert stats[i, K + 1, 0] == 0, "an element in 'other'"
            assert stats[i, 0, 0] == (want[i] == 0).sum()
            for k in range(1, K + 1):
                ys, xs = np.nonzero(want[i] == k)
                assert stats[i, k, 0] == ys.size, (i, k)
                if k <= counts[i]:  # the box is half open: [x0, x1) x [y0, y1)
                    assert ys.size > 0 and stats[i, k, 1:].tolist() == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], (i, k, stats[i, k])
                else:  # an image with fewer components than the batch's largest K: the id does not occur
                    assert not stats[i, k].any()


def test_identities_on_the_device(api, gpu_device):
    import torch

    rng = np.random.default_rng(3)
    lab = np.repeat(np.repeat(rng.integers(0, 3, (3, 25, 33)), 4, axis=1), 4, axis=2).astype(np.uint8)
    lab[rng.integers(0, 2, lab.shape).astype(bool) & (rng.integers(0, 8, lab.shape) == 0)] = 1  # specks and diagonal contacts
    t = torch.from_numpy(lab).to(gpu_device)
    n, H, W = lab.shape
    index = torch.arange(H * W, dtype=torch.int32, device=gpu_device).reshape(H, W)
    for background in (None, 0):
        f4, k4 = api.png_label_components(t, 4, background, "first")
        f8, k8 = api.png_label_components(t, 8, background, "first")
        # exactly K elements are their component's FIRST
        assert (f4 == index).sum(dim=(1, 2)).tolist() == k4.tolist() and (f8 == index).sum(dim=(1, 2)).tolist() == k8.tolist()
        assert (k8 <= k4).all() and (k8 < k4).any()
        # the 8-partition is a coarsening of the 4-partition: a 4-component lies in one 8-component
        for i in range(n):
            pairs = torch.unique(torch.stack([f4[i].reshape(-1), f8[i].reshape(-1)]), dim=1)
            assert pairs.shape[1] == int(k4[i]) + (1 if background is not None and (f4[i] < 0).any() else 0)
        # flipping the input flips the partition: the consecutive ids of the flipped input, flipped back, name the same sets
        c, kc = api.png_label_components(t, 8, background)
        cf, kf = api.png_label_components(torch.flip(t, dims=(1, 2)).contiguous(), 8, background)
        back = torch.flip(cf, dims=(1, 2))
        assert kc.tolist() == kf.tolist()
        for i in range(n):
            pairs = torch.unique(torch.stack([c[i].reshape(-1), back[i].reshape(-1)]), dim=1)
            assert pairs.shape[1] == int(kc[i]) + (1 if (c[i] == 0).any() else 0) and ((pairs[0] == 0) == (pairs[1] == 0)).all()
