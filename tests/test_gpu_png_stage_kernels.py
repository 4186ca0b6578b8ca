"""The twenty-two tensor-stage launchers whose kernels loop over their tasks (include/debig_hip.h: debig_hip_apng_composite_batch,
debig_hip_png_resize / _resize_alpha / _resize_cubic / _resize_color / _label_gather / _color_label / _warp / _warp_color /
_label_warp / _color_label_warp / _tone_hist / _tone_apply / _blur _batch, and the four warp launchers again under the projective
and the elastic map: _persp / _persp_color / _label_persp / _color_label_persp, _elastic / _elastic_color / _label_elastic /
_color_label_elastic) called DIRECTLY on the MI355X, with fewer workgroups than
tasks (DEBIG_STAGE_GRID) and with tiles and runs the host never cuts.  The whole-call tests give every workgroup exactly one task,
so the top-of-task barriers, the tables and counters the kernels keep in LDS from one task to the next and the task shapes beyond
the host's otherwise run on the CPU emulator only, which runs one workgroup at a time and knows nothing of the machine's memory
model.

  * test_battery runs the emulator batteries (tests/test_emu_png_*.py, tests/test_emu_apng.py) as they are -- the same run*() /
    _check() / check() functions, shapes, grids and BIT FOR BIT comparisons with the numpy restatements (png_resize_ref,
    png_alpha_ref, png_filter_ref, png_color_ref, png_warp_ref, png_label_ref, png_color_label_ref, png_color_label_warp_ref,
    png_tone_ref, png_blur_ref, png_persp_ref, png_elastic_ref, apng_ref) -- with the launch seam tests/stage_launch.py switched to the product library.  Nothing
    is compared with the emulator's output; the emulator library is neither built nor loaded.  The persp and elastic batteries
    (MAPPED) go through the runners of the warp batteries (tests/map_launch.py); every case of theirs outside FULL_GRID must have
    launched with fewer workgroups than tasks, and the elastic battery has one workgroup alternate between two files' fields.
    Their cases are collected in tests/test_gpu_png_persp_kernels.py and tests/test_gpu_png_elastic_kernels.py, under the ids they
    have had since they were written; tables, sets and assertions are this file's (MODULES, EXCLUDED, ..., run_case).
  * the *_kept_and_replaced cases order the tasks so that one workgroup both keeps a table for the next task and replaces it, and
    assert from the task list that it does; test_tone_hist_flat_beside_noisy_in_one_workgroup is about the histogram counters of
    all four wavefronts; test_blur_other_tiles_through_few_workgroups joins other tiles than the host's with few workgroups.
  * the test_whole_call_* cases decode a mixed batch through each call family with DEBIG_STAGE_GRID unset and 3: byte-identical.
  * debig_hip_gather, which no other test calls directly, against numpy slicing.

LEFT OUT of the GPU run on purpose (EXCLUDED, checked by test_every_battery_case_runs_or_is_excluded):
  * the tasks that break a bound (`spoil=`, the hand-made bad tasks): they are wrong on purpose, the predicates that refuse them
    are integer checks that do not depend on the machine, and a wrong predicate on a shared GPU would be an out-of-range access.
    The emulator under ASan is their place.  What test_emu_png_blur.test_the_remaining_bounds runs WITHIN the bounds (a 64 x 9
    tile, k at both ends of its range) runs here as test_blur_tasks_at_the_limits.
  * the ASan runs of the emulator (child processes; no GPU code).

RUN ELSEWHERE (ELSEWHERE, checked by the same test): the index de-filter cases of test_emu_png_labels.py.  The four
debig_hip_png_spec_defilter* launchers start one workgroup per task and have no task loop, so DEBIG_STAGE_GRID is not their subject;
they are in the same seam without a grid (stage_launch.NO_GRID), and tests/test_gpu_png_defilter_kernels.py runs their batteries on
the GPU -- tests/test_emu_png_spec.py, test_emu_png_out_format.py, test_emu_png_planar.py and those index cases, past the wrap of
the scratch ring and with rows long enough for the mid-row wait.  The tuned 8-bit de-filter has its own battery, run in every
launch mode by tests/test_gpu_png_defilter_battery.py.  The inflate and the checksum kernels have no task loop either; the
checksum kernel has its own battery (tests/checksum_battery.py: every alignment, tile and modulus edge, spans of one value inside
the other, a grid past 65 535), run on the GPU by tests/test_gpu_checksum.py."""
import ctypes as C
import importlib
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_launch as SL  # noqa: E402

pytestmark = pytest.mark.gpu

# emulator module -> the launchers its run*() functions reach
MODULES = {
    "test_emu_apng": {"apng_composite"},
    "test_emu_png_resize": {"png_resize"},
    "test_emu_png_resize_alpha": {"png_resize_alpha"},
    "test_emu_png_resize_filter": {"png_resize_cubic"},
    "test_emu_png_color": {"png_resize_color", "png_warp_color"},
    "test_emu_png_labels": {"png_label_gather"},
    "test_emu_png_color_labels": {"png_color_label"},
    "test_emu_png_warp": {"png_warp", "png_label_warp"},
    "test_emu_png_color_labels_warp": {"png_color_label_warp"},
    "test_emu_png_tone": {"png_tone_hist", "png_tone_apply"},
    "test_emu_png_blur": {"png_blur"},
    "test_emu_png_persp": {"png_persp", "png_persp_color", "png_label_persp", "png_color_label_persp"},
    "test_emu_png_elastic": {"png_elastic", "png_elastic_color", "png_label_elastic", "png_color_label_elastic"},
}
MAPPED = ("test_emu_png_persp", "test_emu_png_elastic")
BOUND = "hands the kernel tasks that break a bound on purpose"
ASAN = "the emulator under ASan in a child process: no GPU code"
INDEX = "debig_hip_png_spec_defilter_index_batch (one workgroup per task, no task loop): tests/test_gpu_png_defilter_kernels.py"
EXCLUDED = {
    "test_emu_apng::test_kernel_under_address_sanitizer": ASAN,
    "test_emu_png_resize::test_kernel_under_address_sanitizer": ASAN,
    "test_emu_png_resize_alpha::test_kernel_under_address_sanitizer": ASAN,
    "test_emu_png_resize_filter::test_kernel_under_address_sanitizer": ASAN,
    "test_emu_png_labels::test_kernels_under_address_sanitizer": ASAN,
    "test_emu_png_color_labels::test_kernel_under_address_sanitizer": ASAN,
    "test_emu_png_resize_alpha::test_mismatched_tasks_are_skipped": BOUND,
    "test_emu_png_resize_filter::test_mismatched_tasks_are_skipped": BOUND,
    "test_emu_png_color::test_tasks_and_records_that_break_a_bound_are_skipped": BOUND,
    "test_emu_png_labels::test_gather_skips_tasks_that_break_a_bound": BOUND,
    "test_emu_png_color_labels::test_tasks_that_break_a_bound_are_skipped": BOUND,
    "test_emu_png_warp::test_tasks_that_break_a_bound_are_skipped": BOUND,
    "test_emu_png_color_labels_warp::test_tasks_that_break_a_bound_are_skipped": BOUND,
    "test_emu_png_tone::test_tasks_that_break_a_bound_are_skipped": BOUND,
    "test_emu_png_blur::test_tasks_that_break_a_bound_are_skipped": BOUND,
    "test_emu_png_blur::test_the_remaining_bounds": BOUND + " (its tasks within the bounds: test_blur_tasks_at_the_limits)",
    "test_emu_png_persp::test_tasks_that_break_a_bound_are_skipped": BOUND,
    "test_emu_png_elastic::test_tasks_that_break_a_bound_are_skipped": BOUND,
}
# not left out: cases of a module of MODULES about a launcher of another GPU module, which runs them
ELSEWHERE = {
    "test_emu_png_labels::test_index_defilter_every_label_format": INDEX,
    "test_emu_png_labels::test_index_defilter_every_filter_type_and_widths_1_to_70": INDEX,
    "test_emu_png_labels::test_index_past_the_palette_and_other_colour_types_fail_the_task": INDEX,
    "test_emu_png_labels::test_heights_past_the_ring_wrap": INDEX,
    "test_emu_png_labels::test_long_rows_across_bands": INDEX,
}
# tests of a module's own sources and of the restatement: they launch nothing, here as there
NO_LAUNCH = {"test_emu_png_blur::test_the_sources_take_every_path_of_the_rule", "test_emu_png_tone::test_the_sources_take_every_path_of_the_rule",
             "test_emu_png_warp::test_the_special_matrices_hit_what_they_are_for",
             "test_emu_png_persp::test_the_special_matrices_hit_what_they_are_for", "test_emu_png_elastic::test_the_special_fields_hit_what_they_are_for"}
# the cases of the MAPPED batteries whose launches all start one workgroup per task
FULL_GRID = {"test_emu_png_persp::test_numerators_near_2_48_over_the_smallest_denominator",
             "test_emu_png_persp::test_far_positions_are_border_or_an_edge_pixel",
             "test_emu_png_persp::test_uint_bilinear_against_the_rounded_float64_map",
             "test_emu_png_persp::test_the_label_pick_is_the_image_nearest_pick", "test_emu_png_elastic::test_the_label_pick_is_the_image_nearest_pick"}
# the cases that compare with the OUTPUT of the warp kernels launch those as well
WARPS = {"png_warp", "png_warp_color", "png_label_warp", "png_color_label_warp"}
ALSO_WARP = {"test_emu_png_persp::test_affine_matrices_give_the_output_of_the_warp_kernels": WARPS,
             "test_emu_png_elastic::test_no_field_and_zeros_give_the_output_of_the_warp_kernels": WARPS}


def _battery_tests():
    """{"module::test": function} of every test function the emulator modules define"""
    out = {}
    for mod in MODULES:
        m = importlib.import_module(mod)  # (imports neither build nor load the emulator)
        for name, fn in vars(m).items():
            if name.startswith("test") and inspect.isfunction(fn) and fn.__module__ == mod:
                out["%s::%s" % (mod, name)] = fn
    return out


def _param_sets(fn):
    """the argument sets of a test function's parametrize marks, as pytest crosses them"""
    sets = [{}]
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [s.strip() for s in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
        sets = [dict(s, **dict(zip(names, v if len(names) > 1 else (v,)))) for v in mark.args[1] for s in sets]
    return sets


def _word(v):
    return "x".join(_word(e) for e in v) if isinstance(v, (tuple, list)) else str(v)


def _cases(mods=None):
    """the cases of the modules `mods` (default: all of MODULES).  The cases of a MAPPED module keep the ids they have always had,
    the bare test name, in tests/test_gpu_png_persp_kernels.py and tests/test_gpu_png_elastic_kernels.py, which hold nothing else"""
    out = []
    for key, fn in _battery_tests().items():
        mod = key.split("::")[0]
        if key in EXCLUDED or key in ELSEWHERE or mod not in (MODULES if mods is None else mods):
            continue
        stem = key.split("::test_")[1] if mod in MAPPED else key.replace("test_emu_", "").replace("::test_", ":")
        for kw in _param_sets(fn):
            assert set(kw) == set(inspect.signature(fn).parameters), (key, "an argument that no parametrize mark gives")
            out.append(pytest.param(key, kw, id=stem + "".join("-" + _word(v) for v in kw.values())))
    return out


@pytest.fixture(autouse=True)
def on_the_gpu(gpu_device, monkeypatch):
    """every launch of this module's tests goes to the product library, and is recorded: [(kernel, tasks, n, grid)]"""
    monkeypatch.setattr(SL, "backend", "gpu")
    monkeypatch.setattr(SL, "record", [])
    monkeypatch.delenv("DEBIG_STAGE_GRID", raising=False)
    return SL.record


def test_every_battery_case_runs_or_is_excluded():
    tests = _battery_tests()
    ran = {c.values[0] for c in _cases()}
    assert ran | set(EXCLUDED) | set(ELSEWHERE) == set(tests) and not ran & (set(EXCLUDED) | set(ELSEWHERE)) and not set(EXCLUDED) & set(ELSEWHERE)
    assert all(EXCLUDED[k] for k in EXCLUDED) and all(ELSEWHERE[k] for k in ELSEWHERE) and NO_LAUNCH <= ran
    # every launcher of the header with a task loop belongs to a module whose cases run; the four without: test_gpu_png_defilter_kernels.py
    assert set().union(*MODULES.values()) == set(SL.KERNELS) - SL.NO_GRID and len(SL.KERNELS) == 22 + 4 and len(SL.NO_GRID) == 4
    for mod in MODULES:
        assert sum(k.startswith(mod + "::") for k in ran) >= (10 if mod in MAPPED else 1), mod


def run_case(key, kw, on_the_gpu):
    _battery_tests()[key](**kw)
    mod = key.split("::")[0]
    names = {r[0] for r in on_the_gpu}
    assert names <= MODULES[mod] | ALSO_WARP.get(key, set())
    assert bool(names & MODULES[mod]) != (key in NO_LAUNCH), (key, "no launch reached the GPU")
    if mod in MAPPED and key not in NO_LAUNCH | FULL_GRID:
        assert any(0 < g < n for k, _, n, g in on_the_gpu if k in MODULES[mod]), (key, "no launch with fewer workgroups than tasks")


@pytest.mark.parametrize("key,kw", _cases([m for m in MODULES if m not in MAPPED]))
def test_battery(key, kw, on_the_gpu):
    run_case(key, kw, on_the_gpu)


# ---- tables and counters held from one task to the next ------------------------------------------------------------------------

def _transitions(tasks, n, grid, key):
    """[(kept, replaced)] per workgroup of a launch of the first n tasks with `grid` workgroups: how often its next task has the key
    of the one before / another; key(task) is None for a task that uses no table"""
    out = []
    for wg in range(grid):
        held, kept, replaced = None, 0, 0
        for ti in range(wg, n, grid):
            k = key(tasks[ti])
            if k is None:
                continue
            if held is not None:
                kept += k == held
                replaced += k != held
            held = k
        out.append((kept, replaced))
    return out


def _assert_both(record, kernel, grid, key):
    """every launch of `kernel` in the record ran with `grid` workgroups, and ONE of them both kept its table for a next task and
    replaced it for another"""
    seen = [r for r in record if r[0] == kernel]
    assert seen
    for _, tasks, n, g in seen:
        assert g == grid and n > grid
        per_wg = _transitions(tasks, n, grid, key)
        assert any(kept > 0 and replaced > 0 for kept, replaced in per_wg), (kernel, grid, per_wg)


def _shuffled(seed, keep_first=lambda t: False):
    """a spoil= hook that changes no task, only the order: a seeded permutation (tasks for which keep_first holds stay in front,
    as the histogram launch takes a prefix of the list)"""
    def spoil(tasks, *_):
        rng = np.random.default_rng(seed)
        front = [t for t in tasks if keep_first(t)]
        back = [t for t in tasks if not keep_first(t)]
        tasks[:] = [front[i] for i in rng.permutation(len(front))] + [back[i] for i in rng.permutation(len(back))]
    return spoil


@pytest.mark.parametrize("order", ["by_file", "shuffled"])
@pytest.mark.parametrize("grid", [1, 2])
def test_blur_weights_kept_and_replaced(grid, order, on_the_gpu):
    """nine tiles per file, eleven files, six weight tables: in file order a workgroup keeps its weights for the tiles of a file and
    replaces them at the next Gaussian file; shuffled, it mostly replaces them"""
    import test_emu_png_blur as E

    size, ch = E.SIZES[1], 3
    files = E._files(size, ch)
    got, n, _ = E.run(files, size, "float32", "chw", grid=grid, spoil=_shuffled(5) if order == "shuffled" else None)
    assert n == 9 * len(files)
    _assert_both(on_the_gpu, "png_blur", grid, lambda t: t.table_off if t.op == E.B.GAUSSIAN else None)
    for i in range(len(files)):
        assert got[i].tobytes() == E._want(size, ch, i, "float32", "chw").tobytes(), (grid, order, i)


@pytest.mark.parametrize("tile", [(64, 64), (5, 17), (32, 64)])
@pytest.mark.parametrize("grid", [1, 3])
def test_blur_other_tiles_through_few_workgroups(grid, tile, on_the_gpu):
    """the two things the host never does, together: tiles of other shapes than 32 x 32 (the longest last pass a task can have,
    and 85 items for 256 lanes), shuffled, through one and three workgroups; the files whose rows with the halo fit, as
    test_emu_png_blur.test_other_tiles_than_the_hosts takes them"""
    import test_emu_png_blur as E

    size, ch = E.SIZES[1], 2
    th, tw = min(tile[0], size[0]), min(tile[1], size[1])
    idx = [i for i, f in enumerate(E._files(size, ch))
           if (th + 2 * (f[2] // 2 or 1)) * (tw + 2 * (f[2] // 2 or 1)) * ch <= E.PX_CAP and
           (f[1] != E.B.GAUSSIAN or (th + 2 * (f[2] // 2)) * tw * ch <= E.H16_CAP)]
    files = [E._files(size, ch)[i] for i in idx]
    assert len(files) >= 8 and sum(f[1] == E.B.GAUSSIAN for f in files) >= 3
    got, n, _ = E.run(files, size, "float16", "hwc", tile=tile, grid=grid, spoil=_shuffled(8))
    _assert_both(on_the_gpu, "png_blur", grid, lambda t: t.table_off if t.op == E.B.GAUSSIAN else None)
    for k, i in enumerate(idx):
        assert got[k].tobytes() == E._want(size, ch, i, "float16", "hwc").tobytes(), (grid, tile, i)


def test_blur_tasks_at_the_limits():
    """the tasks of test_emu_png_blur.test_the_remaining_bounds that are within the bounds: radius 31 on 64 x 9 tiles of 4 channels
    (35,784 of the 35,840 bytes), and sharpness factors of 16 and -16"""
    import test_emu_png_blur as E

    size, ch = E.SIZES[1], 4
    files = E._files(size, ch)
    assert 126 * 71 * 4 <= E.PX_CAP < 126 * 72 * 4
    got, n, _ = E.run(files[1:2], size, "uint", "hwc", tile=(64, 9), grid=3)
    assert n == 2 * 8 and np.array_equal(got[0], E._want(size, ch, 1, "uint", "hwc"))
    for k in (16 << 16, -(16 << 16)):
        def spoil_k(tasks, per_file, k=k):
            for j in per_file[0]:
                tasks[j].k = k
        got, _, _ = E.run(files[9:10], size, "uint", "hwc", spoil=spoil_k)
        assert np.array_equal(got[0], E.B.blur(files[9][0], E.B.SHARPNESS, 0, k / 65536.0))


def _tone_from_hist(E):
    return lambda t: t.op in (E.T.AUTOCONTRAST, E.T.EQUALIZE)


@pytest.mark.parametrize("order", ["by_file", "shuffled"])
@pytest.mark.parametrize("grid", [1, 2])
def test_tone_tables_kept_and_replaced_and_counters_cleared(grid, order, on_the_gpu):
    """19 runs per file, eleven files of every op: the histogram kernel's LDS counters go from a file to the next through the flush,
    the apply kernel keeps its table for a file's runs and rebuilds it (from a histogram or a stored table) at the next"""
    import test_emu_png_tone as E

    size, ch = E.SIZES[1], 3
    files = E._files(size, ch)
    from_hist = _tone_from_hist(E)
    got, hist, n = E.run(files, size, "uint", "hwc", grid=grid, spoil=_shuffled(6, from_hist) if order == "shuffled" else None)
    assert n == 19 * len(files)
    _assert_both(on_the_gpu, "png_tone_hist", grid, lambda t: t.hist_off)
    _assert_both(on_the_gpu, "png_tone_apply", grid, lambda t: (t.op, t.hist_off if from_hist(t) else t.lut_off))
    for k, f in enumerate([f for f in files if f[1] in (E.T.AUTOCONTRAST, E.T.EQUALIZE)]):
        assert np.array_equal(hist[k], E.T.histogram(f[0], 3)), (grid, order, k)
    for i, f in enumerate(files):
        assert got[i].tobytes() == E._want(f, "uint", "hwc").tobytes(), (grid, order, i)


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("run_len", [4096, 1100])
@pytest.mark.parametrize("order", ["by_file", "shuffled"])
def test_tone_hist_flat_beside_noisy_in_one_workgroup(order, run_len, ch, on_the_gpu):
    """flat images -- every counted byte of a channel in ONE bin, so all four wavefronts pile onto one LDS counter each -- between
    noisy ones, all runs through one workgroup: a counter that the flush leaves uncleared for some wavefront lands in the next
    file's histogram.  A lane counts 16 bytes per round, so a run of the host's 256 pixels keeps wavefront 0 alone busy: the runs
    here are long enough for all four (4096 pixels: one byte per pixel still makes 256 units) or for three and a part"""
    import test_emu_png_tone as E

    size = E.SIZES[1]
    T = E.T
    rng = np.random.default_rng(40 + ch)
    noise = [rng.integers(0, 256, size + (ch,), dtype=np.uint8) for _ in range(2)]
    flat = [np.full(size + (ch,), v, np.uint8) for v in (77, 0, 255)]
    files = [(flat[0], T.EQUALIZE, 0, None), (noise[0], T.EQUALIZE, 0, None), (flat[1], T.AUTOCONTRAST, 0, None),
             (noise[1], T.AUTOCONTRAST, 0, None), (flat[2], T.EQUALIZE, 0, None)]
    cc = T.colour_channels(ch)
    got, hist, n = E.run(files, size, "uint", "chw", run_len=run_len, grid=1, spoil=_shuffled(7) if order == "shuffled" else None)
    assert n == len(files) * -(-size[0] * size[1] // run_len) and run_len * ch // 16 > (192 if run_len == 4096 or ch > 1 else 64)
    _assert_both(on_the_gpu, "png_tone_hist", 1, lambda t: t.hist_off)
    for k, f in enumerate(files):
        want = T.histogram(f[0], cc)
        assert np.array_equal(hist[k], want), (order, k, np.argwhere(hist[k] != want)[:4])
        if k in (0, 2, 4):
            assert (np.count_nonzero(want, axis=1) == 1).all() and int(want.max()) == size[0] * size[1]
        assert got[k].tobytes() == E._want(f, "uint", "chw").tobytes(), (order, k)


def _label_jobs(maps_of):
    """(source index, box, map index) jobs whose tasks, three per job, let a workgroup keep a map and then replace it"""
    import test_emu_png_color_labels as E

    return [(0, None, maps_of[0]), (1, None, maps_of[1]), (0, E.BOXES[2], maps_of[2]), (1, E.BOXES[3], maps_of[3]), (0, None, maps_of[4]),
            (0, None, maps_of[5]), (1, E.BOXES[1], maps_of[6])]


@pytest.mark.parametrize("grid", [1, 2])
def test_color_label_maps_kept_and_replaced(grid, on_the_gpu):
    """three maps, two of one size: tasks of one job keep the map, the next job brings another (or the same one again)"""
    import test_emu_png_color_labels as E

    S = E._sources()
    maps = [E._values(S["c7"][:3], "int64", 1), E._values(S["c7"][2:5], "int64", 2), E._values(S["c2300"][:300], "int64", 4)]
    jobs = _label_jobs([0, 1, 0, 2, 1, 1, 2])
    E.check([S["blocky"], S["noisy"]], jobs, (9, 33), "int64", maps, -7, run=4, grid=grid)  # (compares the tensor and `unmatched`)
    _assert_both(on_the_gpu, "png_color_label", grid, lambda t: (t.map_off, t.map_slots))


@pytest.mark.parametrize("grid", [1, 2])
def test_color_label_warp_maps_kept_and_replaced(grid, on_the_gpu):
    import test_emu_png_color_labels_warp as E

    S = E._sources()
    maps = [E._values(S["c7"][:3], "int64", 1), E._values(S["c7"][2:5], "int64", 2), E._values(S["c2300"][:300], "int64", 4)]
    size = (9, 33)
    mw, mb = E._mats(37, 29, size), E._mats(13, 7, size)
    jobs = [(0, None, 0, mw[2]), (1, None, 1, mw[3]), (0, E.BOXES[2], 0, mb[2]), (1, E.BOXES[2], 2, mb[1]), (0, None, 1, mw[4]),
            (0, None, 1, mw[0]), (1, None, 2, mw[1])]
    E.check([S["blocky"], S["noisy"]], jobs, size, "int64", maps, -7, E.CLAMP, 0, run=4, grid=grid)
    _assert_both(on_the_gpu, "png_color_label_warp", grid, lambda t: (t.map_off, t.map_slots))


@pytest.mark.parametrize("grid", [1, 2])
def test_label_gather_lut_across_sources_and_tables(grid, on_the_gpu):
    """the LUT is staged once per workgroup and serves every task behind it: tasks of two sources and seven boxes (so of other index
    tables), three per job, through one and two workgroups"""
    import test_emu_png_labels as E

    rng = np.random.default_rng(3)
    srcs = [E._sources()[1], rng.integers(0, 256, size=(70, 45)).astype(np.uint8)]
    jobs = [(k % 2, b) for k, b in enumerate(E.BOXES)]
    for dtype, lut in (("int64", E.LUT), ("uint8", E.LUT + 100)):
        got = E.run_gather(srcs, jobs, (9, 33), dtype, lut, run=4, grid=grid)
        for k, (si, box) in enumerate(jobs):
            exp = E.LR.gather(srcs[si].astype(np.uint32), (9, 33), box, lut, dtype)
            assert got[k].dtype == exp.dtype and got[k].tobytes() == exp.tobytes(), (grid, dtype, k)
    _assert_both(on_the_gpu, "png_label_gather", grid, lambda t: (t.src_off, t.sx_off, t.sy_off))


# ---- the whole calls: the host's own task order under the override ---------------------------------------------------------------

from test_gpu_png_blur import files as blur_files  # noqa: E402,F401  (the fixtures of the calls' own GPU tests)
from test_gpu_png_color import files as color_files  # noqa: E402,F401
from test_gpu_png_color_labels_warp import files as clw_files  # noqa: E402,F401
from test_gpu_png_labels import datas as label_datas  # noqa: E402,F401
from test_gpu_png_tensor import datas as tensor_datas  # noqa: E402,F401
from test_gpu_png_tone import files as tone_files  # noqa: E402,F401


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


def _bytes(v):
    """a result of a call as something == compares byte for byte: tensors and arrays as (dtype, shape, bytes)"""
    import torch

    if isinstance(v, torch.Tensor):
        raw = v.contiguous().view(torch.uint8).cpu().numpy() if v.numel() else np.zeros(0, np.uint8)
        return (str(v.dtype), tuple(v.shape), raw.tobytes())
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, v.tobytes())
    if isinstance(v, (list, tuple)):
        return [_bytes(e) for e in v]
    if isinstance(v, dict):
        return {k: _bytes(e) for k, e in v.items()}
    return v


def _same_under_the_override(monkeypatch, call, n_good):
    """call() with DEBIG_STAGE_GRID unset and 3: statuses, infos, tensors and `unmatched` byte-identical; returns the first result"""
    monkeypatch.delenv("DEBIG_STAGE_GRID", raising=False)
    plain = call()
    monkeypatch.setenv("DEBIG_STAGE_GRID", "3")
    three = call()
    monkeypatch.delenv("DEBIG_STAGE_GRID")
    assert _bytes(three) == _bytes(plain)
    st = plain[0] if not isinstance(plain[0], tuple) else [r[0] for r in plain]
    assert sum(s == 0 for s in st) >= n_good > 3  # more good files than workgroups: each takes several tasks
    return plain


def test_whole_call_tensor_resize(api, tensor_datas, monkeypatch):
    for kw in (dict(mode="rgb", depth=8, dtype="float32", layout="chw"), dict(mode="rgba", depth=16, dtype="uint", layout="hwc", antialias=False)):
        _same_under_the_override(monkeypatch, lambda: api.png_decode_batch_tensor(tensor_datas, (75, 50), fill=3, **kw), len(tensor_datas))


def test_whole_call_tensor_warp_with_colour(api, color_files, monkeypatch):
    import test_gpu_png_color as G

    datas = [d for d, _ in color_files]
    rot = [api.png_warp_matrix(wh, G.WARP_TO, angle=30.0, scale=1.7 + 0.2 * k, translate=(1.5 * k, -2.0)) for k, (_, wh) in enumerate(color_files)]
    for kw in (dict(mode="rgb", dtype="bfloat16", layout="chw"), dict(mode="rgba", depth=16, dtype="uint", layout="hwc")):
        _same_under_the_override(monkeypatch, lambda: api.png_decode_batch_tensor(datas, G.WARP_TO, fill=7, warp=rot, border="constant",
                                                                                  border_value=[1.0, 0.25, 0.0, 0.5][:G.CH[kw["mode"]]],
                                                                                  color=G._matrices(api), **kw), G.N_OK)


def test_whole_call_tone_equalize(api, tone_files, monkeypatch):
    import test_gpu_png_tone as G

    datas = [d for d, _ in tone_files]
    for size, kw in ((G.RESIZE_TO, dict(mode="rgb", dtype="uint", layout="hwc")), (G.RESIZE_TO, dict(mode="rgba", dtype="float16", layout="chw"))):
        _same_under_the_override(monkeypatch, lambda: api.png_decode_batch_tensor(datas, size, fill=7, tone=["equalize"] * len(datas), **kw), 6)


def test_whole_call_gaussian_blur(api, blur_files, monkeypatch):
    import test_gpu_png_blur as G

    datas = [d for d, _ in blur_files]
    for kw in (dict(mode="rgb", dtype="float32", layout="chw"), dict(mode="rgba", dtype="uint", layout="hwc", tone=G.TONES)):
        _same_under_the_override(monkeypatch, lambda: api.png_decode_batch_tensor(datas, G.RESIZE_TO, fill=7, blur=G.BLURS, **kw), G.N_OK)


def test_whole_call_labels_with_a_lut(api, label_datas, monkeypatch):
    import test_gpu_png_labels as G

    for dtype in ("int64", "uint8"):
        _same_under_the_override(monkeypatch, lambda: api.png_decode_batch_labels(label_datas, (75, 50), dtype=dtype, lut=G.LUT, fill=9), 8)


def test_whole_call_colour_labels_with_a_map_per_image(api, monkeypatch):
    import test_gpu_png_color_labels as G

    rng = np.random.default_rng(11)  # (the batch of test_per_image_maps_like_coco_panoptic)
    files, maps = [], []
    for k, (w, h) in enumerate([(64, 65), (333, 129), (5, 300), (1, 1), (64, 65), (45, 70)]):
        ids = rng.choice(1 << 24, size=3 + 2 * k, replace=False).astype(np.uint32)
        colours = np.stack([ids & 255, (ids >> 8) & 255, ids >> 16], axis=-1).astype(np.uint8)
        files.append(G._mask_file(rng, w, h, colours, ("rgb", "rgba", "pal")[k % 3], k % 2))
        maps.append({int(i): int(c) for i, c in zip(ids, rng.integers(1, 134, len(ids)))})
    maps[4] = {}
    del maps[5][next(iter(maps[5]))]
    colors = [G._as_colors(m) for m in maps]
    for dtype, size in (("int64", (75, 50)), ("uint8", (32, 24))):
        out = _same_under_the_override(monkeypatch, lambda: api.png_decode_batch_color_labels(files, size, colors, 0, dtype, fill=5), 6)
        assert out[3][4] == size[0] * size[1] and out[3][5] > 0  # `unmatched` is part of what was compared, and is not all zero


def test_whole_call_colour_label_warp(api, clw_files, monkeypatch):
    import test_gpu_png_color_labels_warp as G

    datas = [d for d, _ in clw_files]
    keys = G._data()["keys"]
    maps = [G._values(keys[i::3], "int64", i) for i in range(len(datas))]
    maps[1] = {}
    ws = G._warps(api, clw_files, (33, 65), 3)
    colors = [G._as_colors(m) for m in maps]
    out = _same_under_the_override(monkeypatch, lambda: api.png_decode_batch_color_labels(datas, (33, 65), colors, -1, "int64", fill=5, warp=ws,
                                                                                          border="constant", border_label=-1), 4)
    assert len(set(out[3])) > 1


def test_whole_call_apng(api, monkeypatch):
    import test_gpu_apng as G

    datas = [d for _, d in G.mixed_batch()]
    for force_general in (False, True):
        _same_under_the_override(monkeypatch, lambda: api.apng_decode_batch(datas, force_general=force_general), len(datas))


# ---- debig_hip_gather -------------------------------------------------------------------------------------------------------------

class Copy(C.Structure):  # include/debig_hip.h: debig_copy
    _fields_ = [("src_off", C.c_uint64), ("dst_off", C.c_uint64), ("len", C.c_uint64)]


LENGTHS = [0, 1, 15, 16, 17, 31, 33, 4095, 4096, 4097]
FILL = 0xEE


def _gather_layout(one_arena):
    """(src arena, dst arena as it starts, copies): every destination residue mod 16 x every source residue mod 4 x LENGTHS, and one
    range of 100,003 bytes; 16 or more sentinel bytes between two destinations.  one_arena: the sources lie behind the destinations
    in the same arena.  Either way the source arena ENDS with the last byte of the last source range."""
    rng = np.random.default_rng(17)
    spans = [(da, sa, ln) for ln in LENGTHS for da in range(16) for sa in range(4)] + [(5, 3, 100003)]
    spans = [spans[i] for i in rng.permutation(len(spans))]
    # the last source range: 7 head bytes, then 256 stores of 16 bytes whose source is 1 byte off a dword, no tail -- the last
    # funnel reads the dword that holds the range's last byte, and the arena ends there
    spans.append((9, 2, 7 + 4096))
    dpos, doffs = 64, []
    for da, _, ln in spans:
        dpos += 16 + (da - dpos - 16) % 16
        doffs.append(dpos)
        dpos += ln
    dst_len = dpos + 64 + (-dpos) % 16
    spos, soffs = (dst_len if one_arena else 0), []
    for _, sa, ln in spans:
        spos += (sa - spos) % 4 + 4 * int(rng.integers(0, 3))
        soffs.append(spos)
        spos += ln
    src = rng.integers(0, 256, spos, dtype=np.uint8)
    dst = np.full(dst_len, FILL, np.uint8)
    if one_arena:
        src[:dst_len] = dst
        dst = src
    copies = (Copy * len(spans))(*[Copy(s, d, ln) for s, d, (_, _, ln) in zip(soffs, doffs, spans)])
    assert {(c.dst_off % 16, c.src_off % 4, c.len) for c in copies} >= {(da, sa, ln) for ln in LENGTHS for da in range(16) for sa in range(4)}
    last = copies[len(spans) - 1]
    assert last.src_off + last.len == len(src) and (last.src_off + 7) % 4 == 1
    return src, dst, copies


@pytest.mark.parametrize("one_arena", [False, True])
def test_gather_against_numpy_slicing(one_arena, native_lib, gpu_device):
    import torch

    src, dst, copies = _gather_layout(one_arena)
    want = dst.copy()
    for c in copies:
        want[c.dst_off: c.dst_off + c.len] = src[c.src_off: c.src_off + c.len]
    assert (want == FILL).sum() >= 16 * len(copies)
    native_lib.debig_hip_gather.restype = C.c_int
    native_lib.debig_hip_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    d_src = torch.from_numpy(src.copy()).to(gpu_device)  # (exactly as long as the arena)
    d_dst = d_src if one_arena else torch.from_numpy(dst.copy()).to(gpu_device)
    d_cp = torch.frombuffer(bytearray(bytes(copies)), dtype=torch.uint8).to(gpu_device)
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    rc = native_lib.debig_hip_gather(d_src.data_ptr(), d_dst.data_ptr(), d_cp.data_ptr(), len(copies), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    got = d_dst.cpu().numpy()
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8]
    if not one_arena:
        assert d_src.cpu().numpy().tobytes() == src.tobytes()
