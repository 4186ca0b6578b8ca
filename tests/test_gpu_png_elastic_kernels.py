"""The four launchers of the elastic deformation (include/debig_hip.h: debig_hip_png_elastic_batch, _elastic_color, _label_elastic,
_color_label_elastic) called DIRECTLY on the MI355X: the emulator battery tests/test_emu_png_elastic.py as it is -- the same
runners, shapes, matrices, fields and BIT FOR BIT comparisons with tests/png_elastic_ref.py -- with the launch seam
(tests/stage_launch.py, through tests/elastic_launch.py) switched to the product library, as tests/test_gpu_png_persp_kernels.py
runs the perspective battery.  Its cases run with row runs the host never cuts, with grids smaller than the task count
(DEBIG_STAGE_GRID) and with one workgroup that alternates between two files' fields, which no whole call does.  Nothing is compared
with the emulator's output; the emulator library is neither built nor loaded.

LEFT OUT on purpose (EXCLUDED): the tasks that break a bound.  They are wrong on purpose, the predicates that refuse them are
integer checks that do not depend on the machine, and a wrong predicate on a shared GPU would be an out-of-range access.  The
emulator, also under ASan + UBSan (tools/asan_png_elastic_emu.sh), is their place."""
import inspect
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_launch as SL  # noqa: E402
import test_emu_png_elastic as EE  # noqa: E402  (imports neither build nor load the emulator)
import test_gpu_png_stage_kernels as GK  # noqa: E402  (how a battery's parametrize marks become cases)

pytestmark = pytest.mark.gpu

ELASTIC = {"png_elastic", "png_elastic_color", "png_label_elastic", "png_color_label_elastic"}
EXCLUDED = {"test_tasks_that_break_a_bound_are_skipped": "hands the kernels tasks that break a bound on purpose"}
NO_LAUNCH = {"test_the_special_fields_hit_what_they_are_for"}
# the cases whose launches all start one workgroup per task
FULL_GRID = {"test_the_label_pick_is_the_image_nearest_pick"}
# the cases that compare with the OUTPUT of the warp kernels launch those as well
ALSO_WARP = {"test_no_field_and_zeros_give_the_output_of_the_warp_kernels": {"png_warp", "png_warp_color", "png_label_warp",
                                                                            "png_color_label_warp"}}


def _tests():
    return {name: fn for name, fn in vars(EE).items() if name.startswith("test") and inspect.isfunction(fn) and fn.__module__ == EE.__name__}


def _cases():
    out = []
    for name, fn in _tests().items():
        if name in EXCLUDED:
            continue
        for kw in GK._param_sets(fn):
            assert set(kw) == set(inspect.signature(fn).parameters), (name, "an argument that no parametrize mark gives")
            out.append(pytest.param(name, kw, id=name.replace("test_", "", 1) + "".join("-" + GK._word(v) for v in kw.values())))
    return out


@pytest.fixture(autouse=True)
def on_the_gpu(gpu_device, monkeypatch):
    """every launch of this module's tests goes to the product library, and is recorded: [(kernel, tasks, n, grid)]"""
    monkeypatch.setattr(SL, "backend", "gpu")
    monkeypatch.setattr(SL, "record", [])
    monkeypatch.delenv("DEBIG_STAGE_GRID", raising=False)
    return SL.record


def test_every_battery_case_runs_or_is_excluded():
    ran = {c.values[0] for c in _cases()}
    assert ran | set(EXCLUDED) == set(_tests()) and not ran & set(EXCLUDED) and NO_LAUNCH <= ran and len(ran) >= 10
    assert len(SL.KERNELS) == 14 and not ELASTIC & set(SL.KERNELS)  # (the seam of the other batteries is as it was)


@pytest.mark.parametrize("name,kw", _cases())
def test_battery(name, kw, on_the_gpu):
    _tests()[name](**kw)
    names = {r[0] for r in on_the_gpu}
    assert names <= ELASTIC | ALSO_WARP.get(name, set())
    assert bool(names & ELASTIC) != (name in NO_LAUNCH), (name, "no launch reached the GPU")
    if name not in NO_LAUNCH | FULL_GRID:
        assert any(0 < g < n for k, _, n, g in on_the_gpu if k in ELASTIC), (name, "no launch with fewer workgroups than tasks")
