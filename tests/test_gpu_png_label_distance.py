"""The label distance on the MI355X (include/decode_png.h: debig_png_label_distance; csrc/png_label_distance_kernel.inc):
  * test_battery runs the emulator battery tests/test_emu_png_label_distance.py as it is -- the same run() / check(), shapes, cuts,
    grids and BIT FOR BIT comparisons with the numpy restatement tests/png_label_distance_ref.py, the g plane after the rows launch
    included -- with the launch seam tests/stage_launch.py switched to the product library, so both kernels also run with fewer
    workgroups than tasks.  Nothing is compared with the emulator, which is neither built nor loaded.  LEFT OUT on purpose: the tasks
    that break a bound, for the reason tests/test_gpu_png_stage_kernels.py gives (wrong on purpose, integer predicates that do not
    depend on the machine, and a wrong predicate on a shared GPU would be an out-of-range access).  The seam checks that the inputs
    and the bytes around every buffer are unchanged.
  * the whole call api.png_label_distance against the restatement on the tensors that png_decode_batch_labels returns plain and
    under warp= with a border label of -1, and that png_decode_batch_color_labels returns with packed colours in int64; tensors made
    in torch, int16 read as uint16, a status that skips an image, DEBIG_STAGE_GRID;
  * the identity png_label_distance(t) <= r * r == png_label_boundary(t, r, "disk", "edge") on the device."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_distance_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
import test_emu_png_label_distance as E  # noqa: E402  (imports neither build nor load the emulator)

pytestmark = pytest.mark.gpu

KERNELS = {E.ROWS, E.COLS_K}
EXCLUDED = {"test_tasks_that_break_a_bound_are_skipped": "hands the kernels tasks that break a bound on purpose"}
# the cases of which at least one launch must start fewer workgroups than it has tasks
FEWER = {"test_every_dtype_width_and_height", "test_strips_and_row_runs_cut_at_every_seam", "test_fewer_workgroups_than_tasks_in_both_orders",
         "test_a_launch_over_half_the_strips_writes_only_those", "test_images_without_tasks_keep_the_pattern"}


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
    for k in KERNELS:
        monkeypatch.setitem(SL.KERNELS, k, (SL.IN, SL.OUT, SL.TASKS))
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
    assert on_the_gpu and {r[0] for r in on_the_gpu} == KERNELS, (name, "a kernel whose launch did not reach the GPU")
    for k in KERNELS:
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
    """api.png_label_distance(t, ...) for every (to, cap, out) against the restatement on the tensor's own bytes; the input stays as it
    was -> the last result as numpy"""
    import torch

    lab = _np(t)
    before = lab.copy()
    brute = {}  # the brute force once per `to`: [(d2, none) per image]
    for to, cap, out in cases:
        got = api.png_label_distance(t, to, cap, out, status=status)
        assert got.device == t.device and got.shape == t.shape and got.dtype == (torch.int32 if out == "squared" else torch.float32)
        assert got.data_ptr() != t.data_ptr()
        if to not in brute:
            brute[to] = [R.d2(im, to) if status is None or status[i] == 0 else None for i, im in enumerate(lab)]
        want = np.stack([np.zeros(lab.shape[1:], R.finish(np.zeros(1), np.zeros(1, bool), cap, out).dtype) if b is None else R.finish(*b, cap, out)
                         for b in brute[to]])
        assert _np(got).tobytes() == want.tobytes(), (to, cap, out, np.argwhere(_np(got) != want)[:5])
    assert _np(t).tobytes() == before.tobytes()
    return _np(got), want


def _fit(api, datas, size, **kw):
    return [api.png_warp_matrix((inf["width"], inf["height"]), size, **kw) for inf in (api.png_info(d)[1] for d in datas)]


def test_labels_plain_and_under_a_warp(api, label_datas):
    st, t, _ = api.png_decode_batch_labels(label_datas, (75, 50), dtype="uint8", fill=9)
    assert sum(s == 0 for s in st) >= 8 and sum(s != 0 for s in st) >= 3
    lab = _np(t)
    to = int(np.bincount(lab[[i for i, s in enumerate(st) if s == 0]].ravel()).argmax())
    got, _ = _whole(api, t, st, [(None, None, "squared"), (to, None, "root"), (None, 16, "root"), (to, 5, "squared")])
    assert all(not got[i].any() for i, s in enumerate(st) if s != 0)
    ws = _fit(api, label_datas, (40, 56), angle=30.0, scale=0.8, translate=(2.0, -1.5))
    st, t, _ = api.png_decode_batch_labels(label_datas, (40, 56), dtype="int64", fill=9, warp=ws, border="constant", border_label=-1)
    lab = _np(t)
    good = [i for i, s in enumerate(st) if s == 0]
    assert sum((lab[i] == -1).any() and (lab[i] != -1).any() for i in good) >= 6  # the border label of -1 is an id like any other
    got, _ = _whole(api, t, st, [(None, None, "squared"), (-1, None, "squared"), (-1, 7, "root")])
    assert sum((got[i] > 1).any() for i in good) >= 6


def test_packed_colours_in_int64(api, clw_files):
    datas = [d for d, _ in clw_files] + [b""]
    st, t, _, _ = api.png_decode_batch_color_labels(datas, (64, 96), None, dtype="int64", fill=5)
    assert st[-1] != 0 and sum(s == 0 for s in st) >= 5
    lab = _np(t)
    colour = int(lab[0, 0, 0])
    assert colour > 255 or (lab > 255).any()
    _whole(api, t, st, [(None, None, "squared"), (colour, None, "root"), (None, 3, "squared")])


def _torch_dtypes():
    import torch

    return {"uint8": torch.uint8, "uint16": torch.int16, "int32": torch.int32, "int64": torch.int64}


@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 24, 33), (1, 70, 130)])
@pytest.mark.parametrize("name", ["uint8", "uint16", "int32", "int64"])
def test_tensors_made_in_torch(api, gpu_device, name, shape):
    import torch

    rng = np.random.default_rng(shape[2])
    small = rng.integers(0, 4, (shape[0], -(-shape[1] // 7), -(-shape[2] // 9)))
    lab = np.repeat(np.repeat(small, 7, axis=1), 9, axis=2)[:, :shape[1], :shape[2]].astype(E.DTYPES[name][1])
    flat = lab.reshape(-1)
    top = int(np.iinfo(lab.dtype).max)
    flat[rng.integers(0, flat.size, max(1, flat.size // 200))] = top  # stray pixels at the top of the dtype
    if name == "int64":
        flat[rng.integers(0, flat.size, 2)] = 2 ** 32 + 3  # ... and ids that share their low word with 3
    host = lab.view(np.int16) if name == "uint16" else lab  # uint16 as the library hands it out where torch has none
    t = torch.from_numpy(host.copy()).to(gpu_device)
    assert t.dtype == _torch_dtypes()[name]
    _whole(api, t, None, [(None, None, "squared"), (top, None, "root"), (None, 16, "root"), (0, 2, "squared"), (2 ** 40, None, "squared")])
    if shape[0] == 3:  # a status that skips the middle image: zeros, and only there
        got = _np(api.png_label_distance(t, 0, None, "root", status=[0, 15, 0]))
        assert got.tobytes() == R.apply(lab, 0, None, "root", [0, 15, 0]).tobytes() and not got[1].any()
        with pytest.raises(ValueError, match="one entry"):
            api.png_label_distance(t, status=[0, 0])
    with pytest.raises(ValueError, match="contiguous"):
        api.png_label_distance(t.transpose(1, 2) if shape[1] > 1 else t.expand(3, 2, 1))
    with pytest.raises(ValueError, match="uint8, uint16"):
        api.png_label_distance(t.to(torch.float32))
    assert api.png_label_distance(t[:0]).shape == (0,) + shape[1:]
    assert api.png_label_distance(t[:0], out="root").dtype == torch.float32


def test_the_grid_override_changes_nothing(api, gpu_device, monkeypatch):
    import torch

    rng = np.random.default_rng(6)
    lab = np.repeat(rng.integers(-1, 5, (6, 30, 20)), 10, axis=2).astype(np.int32)  # four strips and one run of rows per image: 24 and 6 tasks
    t = torch.from_numpy(lab).to(gpu_device)
    monkeypatch.delenv("DEBIG_STAGE_GRID", raising=False)
    plain = api.png_label_distance(t)
    monkeypatch.setenv("DEBIG_STAGE_GRID", "3")
    three = api.png_label_distance(t)
    monkeypatch.delenv("DEBIG_STAGE_GRID")
    assert _np(plain).tobytes() == _np(three).tobytes() == R.apply(lab).tobytes()


@pytest.mark.parametrize("r", [1, 3, 16])
def test_the_identity_with_the_boundary_call_on_the_device(api, gpu_device, r):
    import torch

    rng = np.random.default_rng(r)
    lab = np.repeat(np.repeat(rng.integers(0, 5, (3, 9, 11)), 13, axis=1), 17, axis=2)[:, :100, :170].astype(np.int64)
    lab[2] = 4  # a flat image: no edge, no site
    t = torch.from_numpy(lab).to(gpu_device)
    edge = api.png_label_boundary(t, r, "disk", "edge")
    assert torch.equal(api.png_label_distance(t) <= r * r, edge.bool())
    assert torch.equal(api.png_label_distance(t, cap=17, out="root") <= r, edge.bool()) and edge[:2].any() and not edge[2].any()
