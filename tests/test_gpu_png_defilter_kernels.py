"""The four launchers of the general PNG de-filter (include/debig_hip.h: debig_hip_png_spec_defilter_batch, _fmt_batch, _planar_batch,
_index_batch; csrc/png_spec_kernel.inc) called DIRECTLY on the MI355X.  The kernel is a pipeline of four wavefronts: lane 63 of a band
hands the band's last row to the next wavefront through a four-row scratch ring in global memory (plain stores, wave_mem_fence(), then
the publish in an LDS progress word that the consumer polls; the row comes back through ld_hist_u32()), the "up" bytes of the other
lanes come over a DPP shift (png_lane_above), the rows are aligned with png_funnel, the wavefronts meet in png_wave_sync<4>().  Each of
these has a second, trivial body for the CPU emulator, which runs a workgroup in lock step and has no memory model -- so what the
emulator batteries execute at exactly these steps is not what the machine executes.

  * test_battery runs the emulator batteries tests/test_emu_png_spec.py, test_emu_png_out_format.py, test_emu_png_planar.py and the
    index cases of test_emu_png_labels.py as they are -- the same run_images() / run_index() / _check(), shapes, seeds and BIT FOR BIT
    comparisons with the pure-numpy decoder tests/png_spec_ref.py and the converters on top of it -- with the launch seam
    tests/stage_launch.py switched to the product library.  Nothing is compared with the emulator, which is neither built nor loaded.
    Among them: 4, 5 and 6 bands in every filter unit (the ring wraps), rows of 8 to 72 groups over three bands (the consumer waits in
    mid-row, lane 63's lag of 63 steps), scanline bytes at every residue mod 4, every width 1 .. 130, every output format.  The runners
    assert that the arena comes back unchanged outside the tasks' scratch rings and the output arena outside the images; the seam, that
    the bytes around every buffer and the tasks are unchanged.
  * the data-error cases run too: a filter byte above 4 and a palette index past the palette are statuses the kernel is built to
    report, not tasks that break a bound -- the palette read stays inside the 256-entry LDS table, the other wavefronts leave through
    first_bad.
  * after each case the record of the seam must show launches of exactly the launchers the case is about, each with tasks.

LEFT OUT (EXCLUDED, checked by test_every_battery_case_runs_or_is_excluded): the ASan runs of the emulator (child processes; no GPU
code) and the gather cases of test_emu_png_labels.py, whose GPU run is tests/test_gpu_png_stage_kernels.py."""
import importlib
import inspect
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_launch as SL  # noqa: E402

pytestmark = pytest.mark.gpu

# emulator module -> the launcher its runner reaches
MODULES = {
    "test_emu_png_spec": "png_spec_defilter",
    "test_emu_png_out_format": "png_spec_defilter_fmt",
    "test_emu_png_planar": "png_spec_defilter_planar",
    "test_emu_png_labels": "png_spec_defilter_index",
}
# the cases that compare with the OUTPUT of a twin kernel launch that one as well
ALSO = {
    "test_emu_png_out_format::test_format_zero_equals_the_rgba8_kernel": "png_spec_defilter",
    "test_emu_png_planar::test_equals_the_format_twin_transposed": "png_spec_defilter_fmt",
    "test_emu_png_planar::test_error_statuses_equal_the_format_twin": "png_spec_defilter_fmt",
}
ASAN = "the emulator under ASan in a child process: no GPU code"
GATHER = "debig_hip_png_label_gather_batch: a case of tests/test_gpu_png_stage_kernels.py (run or left out there, with its reason)"
EXCLUDED = {
    "test_emu_png_spec::test_kernel_under_address_sanitizer": ASAN,
    "test_emu_png_out_format::test_kernel_under_address_sanitizer": ASAN,
    "test_emu_png_planar::test_kernel_under_address_sanitizer": ASAN,
    "test_emu_png_labels::test_kernels_under_address_sanitizer": ASAN,
    "test_emu_png_labels::test_gather_every_dtype_size_and_box": GATHER,
    "test_emu_png_labels::test_gather_enlarging_40_times_and_the_identity": GATHER,
    "test_emu_png_labels::test_gather_skips_tasks_that_break_a_bound": GATHER,
}
# the statuses the kernel reports for damaged data: they run here
DATA_ERRORS = {
    "test_emu_png_spec::test_bad_filter_byte_and_palette_index",
    "test_emu_png_out_format::test_errors_under_a_format",
    "test_emu_png_out_format::test_short_palette_and_keys",
    "test_emu_png_planar::test_error_statuses_equal_the_format_twin",
    "test_emu_png_planar::test_short_palette_and_keys",
    "test_emu_png_labels::test_index_past_the_palette_and_other_colour_types_fail_the_task",
}
# the shapes that only this module sends to the GPU, in every module
SHAPES = {"test_heights_past_the_ring_wrap", "test_long_rows_across_bands"}


def _battery_tests():
    """{"module::test": function} of every test function the four emulator modules define"""
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
        names = [s.strip() for s in mark.args[0].split(",")]
        sets = [dict(s, **dict(zip(names, v if len(names) > 1 else (v,)))) for v in mark.args[1] for s in sets]
    return sets


def _cases():
    out = []
    for key, fn in _battery_tests().items():
        if key in EXCLUDED:
            continue
        stem = key.replace("test_emu_", "").replace("::test_", ":")
        for kw in _param_sets(fn):
            assert set(kw) == set(inspect.signature(fn).parameters), (key, "an argument that no parametrize mark gives")
            out.append(pytest.param(key, kw, id=stem + "".join("-" + str(v) for v in kw.values())))
    return out


@pytest.fixture(autouse=True)
def on_the_gpu(gpu_device, monkeypatch):
    """every launch of this module's tests goes to the product library, and is recorded: [(kernel, tasks, n, grid)]"""
    monkeypatch.setattr(SL, "backend", "gpu")
    monkeypatch.setattr(SL, "record", [])
    return SL.record


def test_every_battery_case_runs_or_is_excluded():
    tests = _battery_tests()
    ran = {c.values[0] for c in _cases()}
    assert ran | set(EXCLUDED) == set(tests) and not ran & set(EXCLUDED) and all(EXCLUDED.values())
    assert DATA_ERRORS <= ran and set(ALSO) <= ran
    assert set(MODULES.values()) == SL.NO_GRID and all(SL.KERNELS[k] == (SL.INOUT, SL.OUT, SL.TASKS, SL.OUT) for k in SL.NO_GRID)
    for mod in MODULES:
        assert {"%s::%s" % (mod, s) for s in SHAPES} <= ran, mod
        assert sum(k.startswith(mod + "::") for k in ran) >= 5, mod
    assert "test_emu_png_spec::test_stream_alignment" in ran
    # what the stage-kernel module hands over to this one runs here
    import test_gpu_png_stage_kernels as G

    assert set(G.ELSEWHERE) <= ran and all(k in G._battery_tests() for k in G.ELSEWHERE)


@pytest.mark.parametrize("key,kw", _cases())
def test_battery(key, kw, on_the_gpu):
    _battery_tests()[key](**kw)
    want = {MODULES[key.split("::")[0]]} | ({ALSO[key]} if key in ALSO else set())
    assert on_the_gpu, (key, "no launch reached the GPU")
    assert {r[0] for r in on_the_gpu} == want, (key, "the launchers that ran are not the case's")
    assert all(n > 0 and grid == 0 for _, _, n, grid in on_the_gpu), (key, "a launch without tasks")
